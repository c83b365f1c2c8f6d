"""Float64 restatement of the beam searches of tests/ctc_beam_reference.py and tests/gram_beam_reference.py with commits (a test
helper, not collected): the oracle of tests/test_beam_stream_commit_cpu.py and tests/test_beam_stream_commit_gpu.py.

`search` runs the frame loop of ``ctc_beam_reference.beam_search`` (``gram_beam_reference.beam_search`` with a table) with
hypotheses keyed by their token tuples, the same sums in the same order, and after the frames a schedule names it filters the
beam list as asr_ctc_beam_stream_commit does: with the tokens committed so far `done`, the hypotheses whose tokens after `done`
start with P stay, in their order, and `done` grows by P; if none would stay the commit is refused and nothing changes.  An
action is a token tuple P, "auto" (the longest common prefix of the live hypotheses beyond `done`, which drops nothing), or
("best", hold): the best hypothesis' tokens beyond `done` without its last `hold`, the policy of ``commit_best``.
"""
import functools
import math

import numpy as np

import ctc_beam_reference as ref
import gram_beam_reference as gref
from ctc_beam_reference import NEG, lae
from gram_beam_reference import lae3


def ctc_step(beam, lpt, cands, blank, W):
    """one frame of ctc_beam_reference.beam_search; beam: [(labels, pb, pnb)] best first"""
    lpb = lpt[blank]
    entries = {}
    for h, pb, pnb in beam:
        e = entries.setdefault(h, [NEG, NEG])
        e[0] = lae(e[0], lae(pb, pnb) + lpb)
        if h:
            e[1] = lae(e[1], pnb + lpt[h[-1]])
    for h, pb, pnb in beam:
        tot = lae(pb, pnb)
        for c in cands:
            base = pb if (h and h[-1] == c) else tot
            e = entries.setdefault(h + (c,), [NEG, NEG])
            e[1] = lae(e[1], base + lpt[c])
    scored = []
    for pos, (h, (pb, pnb)) in enumerate(entries.items()):
        tot = lae(pb, pnb)
        if tot > NEG:
            scored.append((-tot, pos, h, pb, pnb))
    scored.sort()
    return [(h, pb, pnb) for _, _, h, pb, pnb in scored[:W]]


def gram_step(beam, lpt, cands, blank, W, spell, uni, big):
    """one frame of gram_beam_reference.beam_search; beam: [(string, pb, pu, pg)] best first"""
    entries = {}
    for s, pb, pu, pg in beam:
        e = entries.setdefault(s, [NEG, NEG, NEG])
        e[0] = lae(e[0], lae3(pb, pu, pg) + lpt[blank])
        if pu > NEG:
            e[1] = lae(e[1], pu + lpt[uni[s[-1]]])
        if pg > NEG:
            e[2] = lae(e[2], pg + lpt[big[s[-2:]]])
    for s, pb, pu, pg in beam:
        tot = lae3(pb, pu, pg)
        for c in cands:
            w = spell[c]
            if not w:
                continue
            e = entries.setdefault(s + w, [NEG, NEG, NEG])
            if len(w) == 1:
                e[1] = lae(e[1], (lae(pb, pg) if s[-1:] == w else tot) + lpt[c])
            else:
                e[2] = lae(e[2], (lae(pb, pu) if s[-2:] == w else tot) + lpt[c])
    scored = []
    for pos, (s, (pb, pu, pg)) in enumerate(entries.items()):
        tot = lae3(pb, pu, pg)
        if tot > NEG:
            scored.append((-tot, pos, s, pb, pu, pg))
    scored.sort()
    return [(s, pb, pu, pg) for _, _, s, pb, pu, pg in scored[:W]]


def total(entry):
    return lae(entry[1], entry[2]) if len(entry) == 3 else lae3(entry[1], entry[2], entry[3])


def common_prefix(tails):
    n = 0
    while tails and all(len(t) > n and t[n] == tails[0][n] for t in tails):
        n += 1
    return tuple(tails[0][:n]) if tails else ()


def search(x, beam_width, top_k, schedule=(), blank=0, gram=None, length=None, lag_at=()):
    """x (T, V) f32 logits of one utterance; schedule [(frames consumed, action)] in order (a frame count may repeat) ->
    dict(done: the committed tokens, tails: [(tokens after done, total)] best first, longest: the longest tail any live
    hypothesis had after any frame, log: [(frames, P, status, margin, best)] with best = total(best) and margin = best -
    total(second) before the commit (inf with one hypothesis), lag: {frames: (length of the best hypothesis, common prefix of
    all)} for `lag_at`)"""
    x = np.asarray(x, np.float32)
    T = x.shape[0] if length is None else int(length)
    lp, cands = ref.candidates(x[:T], blank, top_k, None)
    if gram is None:
        beam = [((), 0.0, NEG)]
        step = ctc_step
        extra = ()
    else:
        spell = [tuple(int(u) for u in row if u >= 0) if row[0] >= 0 else () for row in np.asarray(gram).tolist()]
        extra = (spell, {s[0]: v for v, s in enumerate(spell) if len(s) == 1}, {s: v for v, s in enumerate(spell) if len(s) == 2})
        beam = [((), 0.0, NEG, NEG)]
        step = gram_step
    done, longest, log, lag = (), 0, [], {}
    schedule = list(schedule)
    for t in range(T):
        beam = step(beam, lp[t].tolist(), cands[t], blank, beam_width, *extra)
        longest = max([longest] + [len(e[0]) - len(done) for e in beam])
        if t + 1 in lag_at:
            lag[t + 1] = (len(beam[0][0]), len(common_prefix([e[0] for e in beam])))
        while schedule and schedule[0][0] == t + 1:
            act = schedule.pop(0)[1]
            tails = [e[0][len(done):] for e in beam]
            if isinstance(act, str):
                P = common_prefix(tails)
            elif len(act) == 2 and act[0] == "best":
                P = tuple(tails[0][:max(0, len(tails[0]) - act[1])]) if tails else ()
            else:
                P = tuple(act)
            kept = [e for e, tl in zip(beam, tails) if tl[:len(P)] == P]
            margin = total(beam[0]) - total(beam[1]) if len(beam) > 1 else math.inf
            log.append((t + 1, P, 1 if kept else 0, margin, total(beam[0])))
            if kept:
                beam, done = kept, done + P
    return dict(done=done, tails=[(e[0][len(done):], total(e)) for e in beam], longest=longest, log=log, lag=lag)


def every(T, chunk, action):
    """`action` after every `chunk` frames of T"""
    return [(t, action) for t in range(chunk, T + 1, chunk)]


# ---------------------------------------------------------------------------------------------- the inputs of the GPU tests
CHUNK, HOLD = 20, 8
# (T, V, beam_width, top_k, seeds: one utterance each): the unbounded runs of tests/test_beam_stream_commit_gpu.py.  The seeds
# are those among 1 .. 9 at whose commits the best hypothesis leads the second by more than 10 x the comparison's tolerance
# (tests/test_beam_stream_commit_cpu.py checks that), so that the f32 search takes the same prefixes
LONG_CTC = (600, 12, 8, 6, (3, 4, 5, 9))
LONG_GRAM = (600, 12, 8, 6, (3, 4))
GRAM_U = 4                                        # unigrams of the Gram-CTC runs' table (V - 1 - GRAM_U bigrams)


def long_ctc_logits():
    T, V, _, _, seeds = LONG_CTC
    return np.stack([ref.peaky(np.random.RandomState(s), T, V) for s in seeds], axis=1)


def long_gram_inputs():
    T, V, _, _, seeds = LONG_GRAM
    gram = gref.random_table(V, GRAM_U, 7)
    return np.stack([ref.peaky(np.random.RandomState(s), T, V) for s in seeds], axis=1), gram


@functools.lru_cache(maxsize=None)
def long_runs(family):
    """per utterance of the family's long inputs: `search` under ("best", HOLD) every CHUNK frames.  Its log is the schedule of
    explicit prefixes that the GPU tests replay, and its `longest` sizes their streams."""
    if family == "ctc":
        x, gram = long_ctc_logits(), None
        T, _, W, K, _ = LONG_CTC
    else:
        x, gram = long_gram_inputs()
        T, _, W, K, _ = LONG_GRAM
    return [search(x[:, b], W, K, every(T, CHUNK, ("best", HOLD)), 0, gram) for b in range(x.shape[1])]
