from .ctc import gram_ctc, connectionist_temporal_classification  # noqa: F401
from .ctc import Alignment, ctc_align, gram_ctc_align  # noqa: F401
from .nbest import MWER, ctc_nbest_logp, mwer_loss, mwer_parts  # noqa: F401
from .nbest import gram_ctc_nbest_logp, gram_mwer_loss  # noqa: F401
