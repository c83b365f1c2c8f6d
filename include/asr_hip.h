/* libasr_hip -- C ABI of the MI355X (gfx950) CTC acoustic-model training path.
 *
 * Flat C boundary: raw device pointers, sizes, a hipStream_t passed as void*.  No C++ or torch types.
 * The caller owns every buffer (outputs and workspace are allocated before the call, as the
 * reference's Function objects do: asr/nn/sru.py:348-349,388-393); functions enqueue kernels on the
 * given stream and never synchronise, allocate or free.  Return value: 0 = ok, < 0 = error
 * (-1 bad argument, -2 workspace too small, -3 unsupported shape, -4 launch failure); no exception
 * crosses the boundary.  All tensors are dense row-major unless a pitch argument says otherwise.
 *
 * Each entry point names the reference interface it replaces (paths relative to the reference root).
 */
#ifndef ASR_HIP_H
#define ASR_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int asr_version(void);
/* the 16-bit format of every activation, MFMA operand and weight compute copy of THIS build: 0 = bfloat16 (libasr_hip.so, the default),
 * 1 = IEEE half (libasr_hip_f16.so: the same kernels built with -DASR_ACT_F16 for BASELINE configs[4]'s "fp16 MFMA"; the reference
 * allows float16 convolutions, asr/nn/convolution_2d.py:17-19).  Wherever this header says `bf16` it means that format.  The half build
 * refuses the recurrent entry points (asr_gru_*, asr_sru_*: ASR_ERR_UNSUPPORTED); a train step in half needs loss scaling on the caller's
 * side (the gradient factor of asr_step_control). */
int asr_act_dtype(void);
/* a one-wave kernel that idles for `microseconds` (<= 100000) on `stream`: a timed gap (experiments) */
int asr_stream_delay(void* stream, int microseconds);
/* diagnostic: `blocks` workgroups holding `lds_bytes` of LDS each idle for `microseconds` (<= 200000) on `stream` -- makes CUs
 * temporarily unavailable to launches on other streams (tests of the persistent GRU kernels under partial residency) */
int asr_occupy_cus(void* stream, int microseconds, int lds_bytes, int blocks);
/* diagnostic: the stand-in for a resident collective -- `blocks` workgroups (256 threads, `lds_bytes` of LDS each) that stream
 * buf[0, bytes / 2) into buf[bytes / 2, bytes) (read, add, write; buf 16-B aligned, float32) until `microseconds` (<= 200000) have
 * passed.  The reference has no multi-GPU path ("NCCL call sites: zero"); this measures, on one GPU, what an
 * RCCL ring kernel resident beside a persistent recurrence would cost it. */
int asr_stream_traffic(void* stream, int microseconds, int lds_bytes, int blocks, void* buf, long long bytes);

/* ---------------------------------------------------------------------------------------- CTC family
 * Replaces chainer.functions.connectionist_temporal_classification (call sites run/ctc/cnn/train.py:162,191,
 * run/ctc/sru/train.py:161,191) when label_bigram == NULL, and asr/loss/gram_ctc.py:219-315 (GramCTC /
 * gram_ctc) otherwise.
 *   xs             (T, B, V) f32 pre-softmax activations (the reference passes T arrays (B, V))
 *   label_unigram  (B, Lmax) int32, padded; label_bigram (B, Lmax) int32 with -1 = absent, or NULL
 *   x_len, l_len   (B) int32 or NULL (= T / Lmax)       blank: blank symbol id
 *   loss_per_utt   (B) f32  = -log p(labels | x)         loss_mean: scalar f32 or NULL
 *   workspace      asr_ctc_workspace_bytes(...) bytes; it carries alpha/beta from forward to backward
 * backward: grad (T, B, V) f32 = (softmax - occupancy) * scale * gy, zero rows for t >= x_len
 *   gy: device pointer to one f32 (gy_per_utt = 0) or (B) f32 (gy_per_utt = 1), or NULL (= 1)
 *   scale = 1/B reproduces reduce='mean' (asr/loss/gram_ctc.py:291-292), scale = 1 reduce='no'.
 */
size_t asr_ctc_workspace_bytes(int T, int B, int V, int Lmax, int gram);
int asr_ctc_forward(void* stream, const float* xs, const int32_t* label_unigram, const int32_t* label_bigram,
                    const int32_t* x_len, const int32_t* l_len, int T, int B, int V, int Lmax, int blank,
                    float* loss_per_utt, float* loss_mean, void* workspace, size_t workspace_bytes);
/* The same with the log-sum-exp of every (t, b) row of xs handed in (row_lse[t * B + b], e.g. from asr_layernorm_fwd_lse; NULL: as
 * asr_ctc_forward): the rows pass then only gathers the label entries instead of reading the logits twice. */
int asr_ctc_forward_lse(void* stream, const float* xs, const int32_t* label_unigram, const int32_t* label_bigram,
                        const int32_t* x_len, const int32_t* l_len, int T, int B, int V, int Lmax, int blank, float* loss_per_utt,
                        float* loss_mean, void* workspace, size_t workspace_bytes, const float* row_lse);
int asr_ctc_backward(void* stream, const float* xs, const int32_t* x_len, int T, int B, int V, int Lmax, int gram,
                     const float* gy, int gy_per_utt, float scale, float* grad, const void* workspace,
                     size_t workspace_bytes);
/* forward + backward with gy = 1 in one call (the reference derives both from the same alpha+beta table,
 * asr/loss/gram_ctc.py:276,288-290) */
int asr_ctc_loss_grad(void* stream, const float* xs, const int32_t* label_unigram, const int32_t* label_bigram,
                      const int32_t* x_len, const int32_t* l_len, int T, int B, int V, int Lmax, int blank, float scale,
                      float* loss_per_utt, float* loss_mean, float* grad, void* workspace, size_t workspace_bytes);
/* N-best CTC scoring: the exact log p(h_n | x_b) of N hypotheses per utterance (all paths, not the lower bound a beam search
 * reports) and the gradient of sum_{b,n} gy[b,n] log p(h_n | x_b) -- what expected-error (MWER) training and exact rescoring of
 * an N-best list need.  The reference has no counterpart.  The lattices and the alpha / beta recursion are the loss's (the same
 * code, float64 accumulation); the logit rows are read once per (t, b), whatever N is.
 *   xs, x_len, blank  as above                     hyp (B, N, Lmax) int32 labels, hyp_len (B, N) int32
 *   hyp_len[b][n] < 0   an unused slot: logp -inf.  0: the empty hypothesis, logp = sum_t log softmax(xs[t][b])[blank].
 *                       Values above Lmax act as Lmax.  A hypothesis without a path (x_len[b] < length + adjacent repeats, or a
 *                       label outside [0, V)) has logp -inf.
 *   logp (B, N) f32     log p(h_n | x_b);  for N = 1 it is minus asr_ctc_forward's loss_per_utt
 *   backward: grad (T, B, V) f32 = sum_n gy[b][n] (occupancy_n - softmax), zero rows for t >= x_len[b]; every row is written
 *   once.  gy (B, N) f32; the gy of a slot whose logp is -inf is ignored (it may hold NaN).  The sign is the opposite of
 *   asr_ctc_backward's: this is the gradient of +log p.
 *   workspace  asr_ctc_nbest_workspace_bytes(T, B, V, N, Lmax) bytes (0: the dimensions are refused); it carries alpha / beta of
 *   the B * N lattices from forward to backward.
 * N > 128 (the beam's limit) or a path too long for LDS (where asr_ctc_forward_lse refuses it): ASR_ERR_UNSUPPORTED; a null
 * pointer, a dimension or N <= 0, blank outside [0, V): ASR_ERR_BAD_ARG; a short workspace: ASR_ERR_WORKSPACE -- all before any
 * launch. */
size_t asr_ctc_nbest_workspace_bytes(int T, int B, int V, int N, int Lmax);
int asr_ctc_nbest_forward(void* stream, const float* xs, const int32_t* hyp, const int32_t* hyp_len, const int32_t* x_len, int T,
                          int B, int V, int N, int Lmax, int blank, float* logp, void* workspace, size_t workspace_bytes);
int asr_ctc_nbest_backward(void* stream, const float* xs, const int32_t* x_len, int T, int B, int V, int N, int Lmax,
                           const float* gy, float* grad, const void* workspace, size_t workspace_bytes);
/* The same for Gram-CTC: the exact log p(string_n | x_b) of N strings of characters per utterance, every way of cutting a
 * string into the unigram and bigram tokens of the table summed, and the gradient of sum_{b,n} gy[b,n] log p (DESIGN.md section
 * 21).  The lattice of a string is asr_ctc_forward's Gram-CTC lattice with label_unigram[i] = the token that spells (s[i]) and
 * label_bigram[i] = the token that spells (s[i-1], s[i]), -1 where the table has none: every bigram of the table is offered.
 *   xs, x_len, blank, logp, gy, grad  as in asr_ctc_nbest_*; for N = 1 logp is minus asr_ctc_forward's loss_per_utt on those labels
 *   hyp (B, N, Lmax) int32 characters (the ids asr_gram_ctc_beam_search returns), hyp_len (B, N) int32
 *   gram (V, 2) int32   the inventory, as asr_gram_ctc_beam_search takes it: (u, -1) a unigram token, (u1, u2) a bigram token,
 *                       (-1, -1) the blank or an id that is never emitted.  It alone describes the inventory; it is read on every
 *                       call (an index spelling -> token is built in the workspace).  Its entries are only hashed and compared,
 *                       never used as an index; a row with an entry outside [0, V) (second entry: [-1, V)) spells nothing; of two
 *                       rows with the same spelling the smaller token id is used, on every run.
 *   hyp_len[b][n] < 0   an unused slot: logp -inf.  0: the empty string, logp = sum_t log softmax(xs[t][b])[blank].  Values above
 *                       Lmax act as Lmax.  A string with a character that has no unigram token (a negative or out-of-range
 *                       character included) is treated as an unused slot: logp -inf, no gradient -- a lattice with dead unigram
 *                       nodes is not modelled.  A string without a path (more than 2 x_len[b] characters, ...) has logp -inf.
 *   workspace  asr_gram_ctc_nbest_workspace_bytes(T, B, V, N, Lmax) bytes (0: the dimensions are refused); it carries alpha / beta
 *   of the B * N lattices (3 Lmax + 1 nodes, padded to a multiple of 64) from forward to backward.
 * N outside [1, 128], a path too long for LDS, B * N * padded path length beyond int32, or gram == NULL: ASR_ERR_UNSUPPORTED;
 * another null pointer, another dimension <= 0, blank outside [0, V): ASR_ERR_BAD_ARG; a short workspace: ASR_ERR_WORKSPACE -- all
 * before any launch.  No host synchronisation. */
size_t asr_gram_ctc_nbest_workspace_bytes(int T, int B, int V, int N, int Lmax);
int asr_gram_ctc_nbest_forward(void* stream, const float* xs, const int32_t* hyp, const int32_t* hyp_len, const int32_t* x_len,
                               const int32_t* gram, int T, int B, int V, int N, int Lmax, int blank, float* logp, void* workspace,
                               size_t workspace_bytes);
int asr_gram_ctc_nbest_backward(void* stream, const float* xs, const int32_t* x_len, int T, int B, int V, int N, int Lmax,
                                const float* gy, float* grad, const void* workspace, size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------- log-mel features
 * Replace fft.get_specgram / compute_logmel / compute_deltas (asr/fft.py:52-66, 6-19, 90-99), the per-utterance loop of
 * Processor.extract_batch_features (asr/data/processing.py:67-111) and the Loader's normalisation
 * (asr/data/loaders/base.py:22-24), batched over utterances.
 *   asr_specgram  signals (B, sig_pitch) int16 or f32, lengths (B); frame f of utterance b covers samples
 *                 [f*frame_step, f*frame_step+frame_len) zero padded, pre-emphasised, times window (frame_len);
 *                 nframes (B) frames are produced per utterance.  Writes the power spectrum
 *                 (B, Fmax, nfft/2+1) and/or log(pspec . fbank^T) (B, Fmax, nfilt); nfft a power of two <= 1024.
 *                 nfft = 512 (the reference's frame, asr/data/processing.py:54) with frame_step % 4 == 0, sig_pitch % 4 == 0 and an
 *                 aligned buffer: one frame per wave, 256-point complex radix-4 transform in registers; else one workgroup per frame.
 *   asr_logmel    log-mel of a caller-supplied power spectrum (F, nbins) with fbank (nfilt, nbins)
 *   asr_deltas    (B, Fmax, nfilt) log-mel -> the minibatch x (B, 3, nfilt, Tmax) f32: static / delta / delta-delta,
 *                 T_b = nframes[b] - 2 frames, zero beyond; mean/std (3, nfilt) optional
 */
int asr_specgram(void* stream, const void* signals, int sig_is_f32, const int32_t* lengths, long long sig_pitch, int B,
                 int frame_len, int frame_step, int nfft, double preemph, const float* window, const int32_t* nframes,
                 int Fmax, float* pspec_out, const float* fbank, int nfilt, float* logmel_out);
/*   asr_mel_bands       the sparse form of a mel matrix fbank (nfilt, nbins) (asr/fft.py:68-82 builds triangles: 454 of 10280 entries are
 *                       non-zero at 40 x 257): per filter the first non-zero bin, the band length padded to a multiple of 8, the offset of its
 *                       taps, then the taps -- written ONCE per matrix into a caller-owned table of asr_mel_bands_bytes() bytes (16-byte aligned)
 *   asr_specgram_bands  asr_specgram with that table of ITS fbank (nbins = nfft / 2 + 1): the mel stage touches the bands only; a null table,
 *                       or one whose matrix did not fit it (more than 64 filters / 1024 padded taps), falls back to the dense rows */
size_t asr_mel_bands_bytes(void);
int asr_mel_bands(void* stream, const float* fbank, int nfilt, int nbins, void* table, size_t table_bytes);
int asr_specgram_bands(void* stream, const void* signals, int sig_is_f32, const int32_t* lengths, long long sig_pitch, int B,
                       int frame_len, int frame_step, int nfft, double preemph, const float* window, const int32_t* nframes,
                       int Fmax, float* pspec_out, const float* fbank, int nfilt, float* logmel_out, const void* bands);
int asr_logmel(void* stream, const float* pspec, const float* fbank, long long F, int nbins, int nfilt, float* out);
int asr_deltas(void* stream, const float* logmel, const int32_t* nframes, int B, int Fmax, int nfilt, int Tmax,
               const float* mean, const float* stdv, float* out);

/* optional steps of Processor.extract_batch_features and the Loader's running statistics
 *   asr_cmn_pspec            cepstral mean normalisation in the log-power domain (asr/data/processing.py:86-89), in place
 *                            on the (B, Fmax, nbins) power spectrum, frames < nframes[b]
 *   asr_add_white_noise      signal[b] += trunc(gain[b] * n), n ~ N(0, 1) (asr/data/processing.py:74-78; counter-based
 *                            generator: the distribution matches, NumPy's stream does not), f32 signals in place
 *   asr_augment_specgram     speed / vocal-tract perturbation by nearest-index resampling (asr/fft.py:21-50):
 *                            out[b][f][k] = in[b][int(f speed_b)][min(int(k ratio_b), nbins-1)], f < nframes_out[b]
 *                            (= int(nframes_in[b] / speed_b), computed by the caller), zero beyond
 *   asr_running_stats_update asr/data/loaders/base.py:64-80 for every utterance of x (B, CM, T) f32 in turn (frames
 *                            < lengths[b]); mean / nvar (CM) float64 state, total_before = frames seen so far; also
 *                            writes mean32 and the unbiased std32 = sqrt(nvar / (total - 1)) (:39-41)
 *   asr_normalize_bcmt       x <- (x - mean[cm]) / std[cm] over the whole padded array (:24), in place
 */
int asr_cmn_pspec(void* stream, float* pspec, const int32_t* nframes, int B, int Fmax, int nbins);
int asr_add_white_noise(void* stream, float* signals, const int32_t* lengths, long long pitch, int B, const float* gain,
                        unsigned long long seed);
int asr_augment_specgram(void* stream, const float* pspec_in, const int32_t* nframes_out, const double* speed,
                         const double* ratio, int B, int Fmax_in, int Fmax_out, int nbins, float* pspec_out);
int asr_running_stats_update(void* stream, const float* x, const int32_t* lengths, int B, int CM, int T,
                             long long total_before, double* mean, double* nvar, float* mean32, float* std32);
int asr_normalize_bcmt(void* stream, float* x, const float* mean, const float* stdv, int B, int CM, int T);

/* ---------------------------------------------------------------------------------------- greedy decode + CER
 * The evaluation loop of run/ctc/cnn/dev.py:100-108 and asr/error.py:7-68 for a whole minibatch.
 *   asr_argmax_rows    ids[b][t] = argmax_v logits[t][b][v] (first maximum, as np.argmax), logits (T, B, V) f32
 *   asr_ctc_collapse   per utterance: drop blanks and repeats (asr/error.py:38-47) of ids (B, T), frames < lengths[b]
 *                      (NULL: all T, as the reference), compacted into out (B, T) padded with blank, out_len (B);
 *                      merge_repeats = 0 drops blanks only (the label side, asr/error.py:33-37)
 *   asr_edit_distance  Levenshtein distance of `pairs` (reference, hypothesis) id rows (asr/error.py:7-24, without the
 *                      division by len(r)); dist = len(h) when len(r) == 0.  int32 arithmetic (the reference's uint8
 *                      table is defined up to 255 tokens)
 */
int asr_argmax_rows(void* stream, const float* logits, int T, int B, int V, int32_t* ids);
int asr_ctc_collapse(void* stream, const int32_t* ids, const int32_t* lengths, int B, int T, int blank, int merge_repeats,
                     int32_t* out, int32_t* out_len);
int asr_edit_distance(void* stream, const int32_t* ref, const int32_t* ref_len, int ref_pitch, const int32_t* hyp,
                      const int32_t* hyp_len, int hyp_pitch, int pairs, int32_t* dist);
/* Edit alignment and N-best consensus: the table of asr_edit_distance with the path kept.  The reference
 * has neither (asr/error.py:7-24 returns one rate).  Lengths are clamped to [0, pitch]; ids beyond a length are never read.
 * Several alignments reach the same distance; the one reported is pinned: from (i, j) = (len(r), len(h)) back to (0, 0),
 * i == 0: insertion; j == 0: deletion; r[i-1] == h[j-1]: match; d[i][j] == d[i-1][j-1] + 1: substitution;
 * d[i][j] == d[i-1][j] + 1: deletion; otherwise insertion.
 *   asr_edit_align   per (reference, hypothesis) pair of `pairs` id rows:
 *        counts     (pairs, 4)          distance, substitutions, deletions, insertions of the pinned path
 *        ref_to_hyp (pairs, ref_pitch)  the hypothesis position aligned to reference position i (match or substitution), -1 where
 *                                       it is deleted and at i >= len(r); may be NULL
 *        hyp_to_ref (pairs, hyp_pitch)  likewise, -1 for an insertion and at j >= len(h); may be NULL
 *        workspace  asr_edit_align_workspace_bytes(pairs, ref_pitch, hyp_pitch) = pairs * (ref_pitch + hyp_pitch - 1) *
 *                   min(ref_pitch, hyp_pitch) bytes (one back-pointer byte per cell, stored diagonal by diagonal); with both
 *                   maps NULL no back-pointers are kept and workspace may be NULL
 *   asr_nbest_pairwise_distance   ids (B, N, pitch), lens (B, N) read in place -> dist (B, N, N), dist[b][i][j] the Levenshtein
 *        distance of slots i and j of utterance b: symmetric, diagonal 0; one workgroup per unordered pair.  A slot with a
 *        negative length is unused: its row and column are 0
 *   asr_nbest_consensus   every used slot j of utterance b is aligned against slot pivot[b] (the reference) by the rule above;
 *        conf (B, pitch) f32: conf[b][l] = sum over j in index order of post[b][j] where slot j's token aligned to position l
 *        equals the pivot's; 0 at l >= the pivot's length, and for the whole row where pivot[b] is outside [0, N) (-1: no
 *        pivot) or names an unused slot.  No atomics: bitwise reproducible.
 *        workspace  asr_nbest_consensus_workspace_bytes(B, N, pitch) = B * N * 2 * pitch * pitch bytes (back-pointers, then one
 *                   agreement byte per slot and position)
 * The sweep holds three diagonals of pitch + 1 ints in LDS: ref_pitch (pitch) > 5460 is ASR_ERR_UNSUPPORTED, as for
 * asr_edit_distance; so are hyp_pitch >= 2^19 (asr_edit_align packs the distance beside a 13-bit count), more than 2^31 - 1
 * workgroups and, for asr_nbest_consensus, B > 65535.  NULL (but for the optional maps) or non-positive arguments:
 * ASR_ERR_BAD_ARG; a short workspace: ASR_ERR_WORKSPACE.  The workspace queries run on the host and return 0 for an empty
 * problem. */
size_t asr_edit_align_workspace_bytes(int pairs, int ref_pitch, int hyp_pitch);
int asr_edit_align(void* stream, const int32_t* ref, const int32_t* ref_len, int ref_pitch, const int32_t* hyp,
                   const int32_t* hyp_len, int hyp_pitch, int pairs, int32_t* counts, int32_t* ref_to_hyp, int32_t* hyp_to_ref,
                   void* workspace, size_t workspace_bytes);
int asr_nbest_pairwise_distance(void* stream, const int32_t* ids, const int32_t* lens, int B, int N, int pitch, int32_t* dist);
size_t asr_nbest_consensus_workspace_bytes(int B, int N, int pitch);
int asr_nbest_consensus(void* stream, const int32_t* ids, const int32_t* lens, const int32_t* pivot, const float* post, int B,
                        int N, int pitch, float* conf, void* workspace, size_t workspace_bytes);
/* CTC prefix beam search: the N-best counterpart of the greedy decode above (xp.argmax at run/ctc/cnn/dev.py:102-106 and
 * run/ctc/cnn/test.py:102, then the collapse of asr/error.py:38-47); the reference has no beam decoder.  Log-space prefix beam
 * search over (T, B, V) f32 pre-softmax logits (the CTC loss's input), frames < lengths[b] (NULL: all T; later frames are never
 * read).  Per frame the candidates are the top_k non-blank ids by value (lower id on equal values; top_k above V - 1 acts as
 * V - 1), those with log-softmax >= min_logp (-INFINITY: no threshold); the beam keeps the beam_width best prefixes by
 * log p = logaddexp(p_blank, p_nonblank), ties to the earlier canonical position.
 *   out_ids   (B, beam_width, T) the final beam sorted by score descending, label ids padded with blank
 *   out_len   (B, beam_width)    labelling lengths; unused slots 0       out_score (B, beam_width) f32 log-probability, unused -inf
 *   workspace asr_ctc_beam_workspace_bytes(T, B, V, beam_width, top_k) bytes
 * beam_width <= 128, top_k <= 64, beam_width * top_k <= 4096, else ASR_ERR_UNSUPPORTED.  Bitwise reproducible. */
size_t asr_ctc_beam_workspace_bytes(int T, int B, int V, int beam_width, int top_k);
int asr_ctc_beam_search(void* stream, const float* logits, const int32_t* lengths, int T, int B, int V, int blank, int beam_width,
                        int top_k, float min_logp, void* workspace, size_t workspace_bytes, int32_t* out_ids, int32_t* out_len,
                        float* out_score);
/* CTC / Gram-CTC forced (Viterbi) alignment: the best path through the lattice of the loss above (the same node labels and edges,
 * built by the same code: label_bigram == NULL is CTC, otherwise Gram-CTC), i.e. which frames belong to which token.  The reference
 * has no aligner (run/gram_ctc/cnn/refine.py:94-107 counts the grams of a per-frame argmax instead).  Arguments up to `blank` as for
 * the loss; xl = min(x_len[b], T) (T if NULL), L = clamp(l_len[b], 0, Lmax) (Lmax if NULL).  Every element of every output is
 * written on every call:
 *   frame_ids (B, T)     token id the best path emits at frame t; blank on blank frames and for t >= xl
 *   n_tok     (B)        tokens of the chosen segmentation (CTC: L; Gram-CTC: ceil(L/2) .. L)
 *   tok_ids, tok_pos, tok_start, tok_end (B, Lmax) int32, tok_logp (B, Lmax) f32, for k < n_tok[b]: the token, the index into
 *                        label_unigram[b] of the first unigram it covers (the bigram label_bigram[b][i] ends at i: its position is
 *                        i - 1), the frames [tok_start, tok_end) it occupies and the sum of its log-softmax over them;
 *                        k >= n_tok[b]: id blank, the rest 0
 *   score     (B)        log-probability of the best path (<= -loss); an utterance without a live path (the loss reports 1e10):
 *                        score -inf, n_tok 0, frame_ids all blank
 * Decisions are taken in float64 on the raw logits; ties go to the smallest diagonal offset, among final nodes to the largest
 * node index.  Bitwise reproducible.  workspace: the bytes the query below names for (T, B, V, Lmax, gram);
 * ASR_ERR_UNSUPPORTED where the loss gives it (path too long for LDS). */
size_t asr_ctc_align_workspace_bytes(int T, int B, int V, int Lmax, int gram);
int asr_ctc_align(void* stream, const float* xs, const int32_t* label_unigram, const int32_t* label_bigram, const int32_t* x_len,
                  const int32_t* l_len, int T, int B, int V, int Lmax, int blank, int32_t* frame_ids, int32_t* tok_ids,
                  int32_t* tok_pos, int32_t* tok_start, int32_t* tok_end, float* tok_logp, int32_t* n_tok, float* score,
                  void* workspace, size_t workspace_bytes);
/* CTC keyword spotting: does utterance b contain keyword k, on which frames, and how sure is the model.  A
 * free-boundary Viterbi search over the keyword's own lattice tok_1, blk_2, tok_2, .., blk_L, tok_L (no leading or trailing blank),
 * K keywords by B utterances per call; the logits are read once whatever K is.  The reference has no keyword search.  This is the
 * CTC form over token ids; asr_gram_kws_detect below searches a spelled phrase over every Gram-CTC decomposition.
 * With xmax[t] the f32 maximum of row t and c(t, v) = (double)x[t][v] - (double)xmax[t], for t in [0, xl), xl = min(lengths[b], T)
 * (NULL: T), every value -inf and every start -1 before the first frame:
 *   tok_1[t] = c(t, w_1)   + best(tok_1[t-1], fresh start (0.0, start = t))
 *   blk_i[t] = c(t, blank) + best(blk_i[t-1], tok_{i-1}[t-1])
 *   tok_i[t] = c(t, w_i)   + best(tok_i[t-1], blk_i[t-1], tok_{i-1}[t-1] only if w_i != w_{i-1})
 * in float64, one addition per step; `best` takes the first maximum in the order written and the start travels with it.
 * Keyword image (asr/spot.py builds it on the host):
 *   uniq (U) i32          the distinct token ids of all keywords (an id outside [0, V) reads as -inf)
 *   node_tok (K, Lmax)    the index into uniq of token i of keyword k; -1 where padded, and everywhere in a keyword without a path
 *   kw_len (K)            tokens of keyword k; a keyword with kw_len outside [1, Lmax] or a node_tok outside [0, U) below kw_len has
 *                         no path: its det is -inf and its starts are -1 everywhere
 * asr_kws_detect -- every element of every output is written on every call:
 *   det (B, K, T) f32         (float)tok_L[t]: the best, over all starts s and all paths of the keyword on frames s..t that begin and
 *                             end on a token, of log p(path) - log p(greedy path on s..t); <= 0; -inf for t >= xl
 *   det_start (B, K, T) i32   the start frame s of that path; -1 where det is -inf
 *   fill (B, T) f32           xmax[t] - lse[t], the greedy path's log-probability of the frame (lse as asr_ctc_align forms it); 0 for
 *                             t >= xl
 *   state                     NULL: one shot.  Otherwise asr_kws_state_bytes(B, K, Lmax) bytes, 8-byte aligned, initialised by
 *                             asr_kws_state_reset (mask (B) i32: only the utterances with a non-zero entry; NULL: all): the call
 *                             continues from the carried node values, starts and frame count of every utterance and stores them
 *                             back; lengths are then the valid frames of this chunk and det_start counts the utterance's own frames
 *                             since its last reset.  However the frames are cut, the outputs over the valid frames are bit for bit
 *                             those of one call.
 *   workspace                 asr_kws_workspace_bytes(T, B, U) bytes
 * asr_kws_hits -- non-maximum suppression per (b, k), up to max_hits rounds: among the frames e < xl whose det is finite, >=
 * min_score (-INFINITY: no threshold) and whose span [det_start[e], e] meets no recorded span, take the largest det (ties: the
 * smaller start, then the larger e) and record it:
 *   hit_start, hit_end (B, K, max_hits) i32   the span [start, end): end = e + 1;   unused slots -1
 *   hit_score, hit_logp (B, K, max_hits) f32  det[e], and (float)((double)det[e] + the float64 sum of fill[start .. e], left to
 *                                             right): the log-probability of the best path of the occurrence; unused slots -inf
 *   n_hits (B, K) i32
 * Lmax > 64 (one wave owns a lattice), max_hits > 4096 and more than 2^31 - 1 workgroups: ASR_ERR_UNSUPPORTED.  NULL (but for
 * lengths, state, mask) or non-positive arguments: ASR_ERR_BAD_ARG.  All checks precede the first launch; no host synchronisation;
 * bitwise reproducible.  The two queries run on the host and return 0 for an empty problem. */
size_t asr_kws_workspace_bytes(int T, int B, int U);
size_t asr_kws_state_bytes(int B, int K, int Lmax);
int asr_kws_state_reset(void* stream, void* state, int B, int K, int Lmax, const int32_t* mask);
int asr_kws_detect(void* stream, const float* logits, const int32_t* lengths, int T, int B, int V, int blank, const int32_t* uniq,
                   int U, const int32_t* node_tok, const int32_t* kw_len, int K, int Lmax, void* state, float* det,
                   int32_t* det_start, float* fill, void* workspace, size_t workspace_bytes);
int asr_kws_hits(void* stream, const float* det, const int32_t* det_start, const float* fill, const int32_t* lengths, int B, int K,
                 int T, int max_hits, float min_score, int32_t* hit_start, int32_t* hit_end, float* hit_score, float* hit_logp,
                 int32_t* n_hits);
/* Gram-CTC keyword spotting over spelled strings: the phrase is a string of characters c_1..c_L (unigram
 * ids), and one lattice holds every way of cutting it into unigram and bigram tokens.  With u_i the token spelled (c_i) and g_i
 * (i >= 2) the token spelled (c_{i-1}, c_i), either of which the inventory may lack, position i has the nodes U_i, G_i (i >= 2)
 * and B_i (the blank between positions i-1 and i, i >= 2); no leading or trailing blank.  c(t, v), xl, the float64 max-plus step
 * and the (-inf, -1) before the first frame are those of asr_kws_detect; an absent node keeps (-inf, -1):
 *   U_1[t] = c(t, u_1)   + best(U_1[t-1], fresh start (0.0, start = t))
 *   G_2[t] = c(t, g_2)   + best(G_2[t-1], fresh start (0.0, start = t))
 *   B_i[t] = c(t, blank) + best(B_i[t-1], U_{i-1}[t-1], G_{i-1}[t-1])                                         i >= 2
 *   U_i[t] = c(t, u_i)   + best(U_i[t-1], B_i[t-1], U_{i-1}[t-1] only if c_i != c_{i-1}, G_{i-1}[t-1])        i >= 2
 *   G_i[t] = c(t, g_i)   + best(G_i[t-1], B_{i-1}[t-1], U_{i-2}[t-1], G_{i-2}[t-1] only if g_i != g_{i-2})    i >= 3
 *   det[t] = (float)best(U_L[t], G_L[t]), det_start[t] the winner's start
 * `best` takes the first maximum in the order written (a later candidate wins only if strictly larger), the start travels with
 * the winner, and a node whose new value is -inf gets start -1.  These are the edges of the Gram-CTC loss lattice with its two
 * guards, minus the outer blanks, plus the fresh starts.  det is the best, over all starts, all decompositions and all paths of a
 * decomposition that begin and end on a token, of log p(path) - log p(greedy path): exactly 0.0 where the greedy path spells the
 * phrase with any mix of unigram and bigram tokens.
 * Image (asr/spot.py: GramKeywordSet builds it on the host):
 *   uniq (U) i32                    the distinct token ids of all phrases, unigram and bigram tokens alike
 *   node_uni, node_big (K, Lmax)    the index into uniq of u_i and of g_i; an index outside [0, U) means the node is absent;
 *                                   node_big[k][0] is always absent.  The guards compare these indices (where a node is absent
 *                                   the guard is moot)
 *   kw_len (K)                      characters of phrase k; outside [1, Lmax] the phrase has no path: det -inf, starts -1
 * det, det_start, fill, lengths, state, workspace (asr_kws_workspace_bytes(T, B, U)) and every refusal are as in asr_kws_detect;
 * the state holds three nodes per position (36 bytes) and has its own query and reset.  asr_kws_hits takes the outputs as they
 * are. */
size_t asr_gram_kws_state_bytes(int B, int K, int Lmax);
int asr_gram_kws_state_reset(void* stream, void* state, int B, int K, int Lmax, const int32_t* mask);
int asr_gram_kws_detect(void* stream, const float* logits, const int32_t* lengths, int T, int B, int V, int blank,
                        const int32_t* uniq, int U, const int32_t* node_uni, const int32_t* node_big, const int32_t* kw_len, int K,
                        int Lmax, void* state, float* det, int32_t* det_start, float* fill, void* workspace,
                        size_t workspace_bytes);
/* Back-off n-gram language model over token ids (order 1-4, natural log, ARPA semantics) and the beam search fused with it
 * (asr/lm.py builds and uploads the image).  The reference has no language model.
 * Image:
 *   uni  (vlm, 2) f32    (logp, backoff) of every id 0 .. vlm - 1: dense.  vlm >= V; <s> and </s>, where used, are ids >= V
 *   keys (slots, 4) i32  the tokens of an n-gram of order 2-4, oldest first, padded with -1; an unused slot is -1 -1 -1 -1
 *   vals (slots, 2) f32  (logp, backoff) of the n-gram in the same slot
 *   slots is 0 (keys, vals NULL: unigrams only) or a power of two; load <= 0.5; linear probing from
 *       h = 0x9E3779B97F4A7C15;  for the four key words k, as uint32:  h = (h ^ k) * 0xBF58476D1CE4E5B9 mod 2^64;  h ^= h >> 32
 *       slot = (uint32)h & (slots - 1)
 *   keys are compared in full; a probe sequence ends at a match, at an unused slot, or after max_probe slots (the builder's
 *   longest displacement + 1), so no table content can make a kernel spin.
 * Step: log P(w | c) with c the last min(order - 1, available) tokens, (bos) first when bos >= 0: the longest suffix of c whose
 * extension by w is in the model gives the log-probability (the unigram when none is).  The f32 sum, in this order: 0, + the
 * backoff of every longer suffix, longest first (0 where that suffix is not in the model), + the log-probability.  A context
 * token outside 0 .. vlm - 1 ends the context there; a scored token outside gives NaN.
 * asr_ngram_score: ids (N, Lmax) i32, lengths (N) or NULL (all Lmax) -> out_tok (N, Lmax) f32 the step of every token (0 past the
 * length), out_sum (N) f32 their sum plus, when eos >= 0, log P(eos | the last tokens).  bos / eos < 0: none.  Bitwise reproducible.
 * asr_ctc_beam_search_lm: asr_ctc_beam_search with every prefix h carrying lm(h) = lm(parent) + step(parent, c) (f32, fixed
 * when the prefix enters the beam) and ranked, in every frame, by  total + (alpha * lm + beta * len)  in f32; ties and merging
 * as in the unfused search (the merged entry keeps the stay's lm).  After the last frame, when eos >= 0, lm += log P(eos | h);
 * the beam is then sorted by  out_score = out_ctc + (alpha * out_lm + beta * len),  ties to the earlier slot.
 *   out_ids, out_len, out_score as asr_ctc_beam_search (out_score: the combined score)
 *   out_ctc (B, beam_width) f32 logaddexp(p_blank, p_nonblank), unused -inf       out_lm (B, beam_width) f32 lm(h), unused 0
 * With alpha = beta = 0 and eos < 0 out_ids, out_len and out_score equal asr_ctc_beam_search's bit for bit.  Model values must
 * be finite.  Limits of asr_ctc_beam_search; order > 4 is ASR_ERR_UNSUPPORTED; order < 1, a slots that is neither 0 nor a power
 * of two, max_probe <= 0 with slots > 0, vlm < V, bos or eos >= vlm are ASR_ERR_BAD_ARG. */
int asr_ngram_score(void* stream, const float* uni, int vlm, const int32_t* keys, const float* vals, int slots, int max_probe,
                    int order, const int32_t* ids, const int32_t* lengths, int N, int Lmax, int bos, int eos, float* out_tok,
                    float* out_sum);
size_t asr_ctc_beam_lm_workspace_bytes(int T, int B, int V, int beam_width, int top_k);
int asr_ctc_beam_search_lm(void* stream, const float* logits, const int32_t* lengths, int T, int B, int V, int blank,
                           int beam_width, int top_k, float min_logp, const float* uni, int vlm, const int32_t* keys,
                           const float* vals, int slots, int max_probe, int order, int bos, int eos, float alpha, float beta,
                           void* workspace, size_t workspace_bytes, int32_t* out_ids, int32_t* out_len, float* out_score,
                           float* out_ctc, float* out_lm);
/* Contextual phrase biasing (asr/bias.py builds and uploads the image): an Aho-Corasick automaton over a
 * list of phrases (token-id sequences without the blank, each with a per-token weight w > 0) runs beside every hypothesis of the
 * beam search, pays a bonus as a match grows and takes it back when the match is abandoned.  The reference has no biasing.
 * Automaton: the trie of the phrases; the weight of the edge into node v is the largest w of the phrases through v; phi(s) the sum
 * of the edge weights from the root to s; fail / goto as usual; out(s) the sum of w * length over every phrase that is a suffix of
 * the string of s; adv(s) = phi(s) - phi(u), u the deepest of s and its trie ancestors at which a phrase ends (the root if none).
 * A step from s on c: s' = goto(s, c), delta = out(s') + adv(s') - adv(s).  bias_open(h) is the left-to-right f32 sum of the deltas
 * along h from the root, bias(h) = bias_open(h) - adv(state(h)): the sum of w * length over every occurrence of every phrase in h.
 * Image (sparse, defaulting to the root):
 *   keys (slots, 2) i32  (state, token) of a stored transition: (0, c) where goto(0, c) != 0, and (s, c), s != 0, where
 *                        goto(s, c) != goto(0, c); an unused slot is -1 -1
 *   vals (slots, 2) i32  (next state, the bit pattern of the f32 delta) of the transition in the same slot
 *   ret  (n_states) f32  -adv(s);  n_states >= 1, state 0 is the root
 *   slots is 0 (keys, vals NULL: no phrases) or a power of two; load <= 0.5; linear probing from the n-gram image's hash over the
 *   key words (state, token, -1, -1); keys are compared in full; a probe sequence ends at a match, at an unused slot, or after
 *   max_probe slots (the builder's longest displacement + 1), so no table content can make a kernel spin.
 * Look-up of (s, c), in f32: a hit at (s, c) gives (next, delta); a miss there and a hit at (0, c) gives (next0, ret[s] + delta0);
 * a miss at both gives (0, ret[s]).  A `next` outside [0, n_states) counts as 0, so no table content causes an out-of-range read.
 * asr_ctx_score: ids (N, Lmax) i32 over [0, V), lengths (N) or NULL (all Lmax) -> out_tok (N, Lmax) f32 the delta of every token
 * (0 past the length), out_sum (N) f32 their left-to-right sum, plus ret[state] when finalize != 0 (bias instead of bias_open).
 * An id outside [0, V) gives NaN for that token and sends the state to the root.  Bitwise reproducible.
 * asr_ctc_beam_search_bias: asr_ctc_beam_search_lm (uni != NULL) or asr_ctc_beam_search (uni == NULL: the other model arguments
 * are ignored and out_lm is all 0) with every prefix carrying bias_open and its state, both fixed when the prefix enters the beam,
 * and ranked, in every frame, by  (total + (alpha * lm + beta * len)) + bias_open  resp.  total + bias_open  in f32.  Merging,
 * canonical positions and tie rules are the parents'; a merged entry keeps the stay's values; pb / pnb stay pure CTC quantities.
 * After the last frame bias = bias_open + ret[state], the eos term goes into lm as in the parent, and the beam is sorted by
 * out_score = (out_ctc + (alpha * out_lm + beta * len)) + out_bias  resp.  out_ctc + out_bias,  ties to the earlier slot.
 *   out_ids, out_len, out_score, out_ctc, out_lm as asr_ctc_beam_search_lm       out_bias (B, beam_width) f32 bias(h), unused 0
 *   workspace asr_ctc_beam_bias_workspace_bytes(T, B, V, beam_width, top_k) bytes
 * Every element of every output is written on every call; an utterance without frames gives the empty hypothesis in slot 0.  With
 * a graph without phrases (n_states 1, slots 0) the outputs equal the parent entry's bit for bit and out_bias is all 0.
 * Limits and error codes of the parent entries; n_states < 1, ret == NULL, a g_slots that is neither 0 nor a power of two,
 * g_max_probe <= 0 or NULL g_keys / g_vals with g_slots > 0 are ASR_ERR_BAD_ARG.  All checks run before the first launch.  Frames
 * past lengths[b] are never read.  No host synchronisation.  Bitwise reproducible. */
int asr_ctx_score(void* stream, const int32_t* g_keys, const int32_t* g_vals, int g_slots, int g_max_probe, const float* g_ret,
                  int g_n_states, int V, const int32_t* ids, const int32_t* lengths, int N, int Lmax, int finalize, float* out_tok,
                  float* out_sum);
size_t asr_ctc_beam_bias_workspace_bytes(int T, int B, int V, int beam_width, int top_k);
int asr_ctc_beam_search_bias(void* stream, const float* logits, const int32_t* lengths, int T, int B, int V, int blank,
                             int beam_width, int top_k, float min_logp, const float* uni, int vlm, const int32_t* keys,
                             const float* vals, int slots, int max_probe, int order, int bos, int eos, float alpha, float beta,
                             void* workspace, size_t workspace_bytes, int32_t* out_ids, int32_t* out_len, float* out_score,
                             float* out_ctc, float* out_lm, const int32_t* g_keys, const int32_t* g_vals, int g_slots,
                             int g_max_probe, const float* g_ret, int g_n_states, float* out_bias);
/* Streaming CTC beam search: asr_ctc_beam_search, asr_ctc_beam_search_lm or asr_ctc_beam_search_bias fed
 * chunk by chunk, the beam carried between the calls in a device-resident state.  For every cutting of the frames into chunks,
 * result after the last chunk is bit for bit the output of the one-shot entry on the concatenated frames (its first min(T, Lcap)
 * id columns), and after every earlier chunk that of the frames so far.  The variant is fixed by what is passed: uni == NULL: no
 * model (the other model arguments are ignored); g_ret == NULL: no graph (the other graph arguments must then be NULL / 0).  The
 * same variant, B, beam_width and max_frames go to every call on one state.
 *   state     asr_ctc_beam_stream_state_bytes(B, beam_width, max_frames, with_lm, with_bias) bytes, 256-byte aligned.  Per utterance
 *             a header (a magic word, B, beam_width, max_frames, the variant, the beam's occupancy, the frames consumed), the
 *             beam's per-prefix fields as arrays of beam_width entries (pb, pnb, hash, parent hash, len, last, parent's last,
 *             node; with a model lm and three context tokens; with a graph bias_open and the automaton state), and the prefix
 *             table of max_frames * beam_width (parent node, token) pairs.  Opaque to the caller; copying the bytes copies the search.
 *   workspace asr_ctc_beam_stream_workspace_bytes(Tc, B, V, beam_width, top_k) bytes: the candidate rows of one chunk, per call
 * reset:   writes the header and the root beam (with a model, its context is (bos); bos < 0: none) of every utterance, or, with
 *          mask (B) int32, of the utterances with mask[b] != 0: a batch slot starts a new utterance while the others go on.
 * advance: consumes logits (Tc, B, V) f32; lengths (B) int32 or NULL (all Tc) is the number of valid frames of this chunk per
 *          utterance: 0 leaves that utterance untouched, frames past it are never read.  frames_before is the sum of Tc over the
 *          advance calls since the last reset of all utterances, the host's upper bound on every utterance's consumed frames;
 *          frames_before + Tc > max_frames is ASR_ERR_UNSUPPORTED.  On the device an utterance never consumes frames beyond
 *          max_frames, whatever it is told, and no node is written outside the table.  blank, top_k, min_logp, alpha and beta as
 *          in the one-shot entries; they should not change within an utterance.
 * result:  the end terms (with a model and eos >= 0, lm += log P(eos | h); with a graph, bias = bias_open + ret[state]), the final
 *          order and the backtrack of the one-shot entry, applied to the saved beam; the state is not changed, so it can be called
 *          after any chunk.  out_ids (B, beam_width, Lcap) padded with blank; out_len, out_score (B, beam_width); out_ctc, out_lm
 *          with a model or a graph, out_bias with a graph (NULL otherwise), as the one-shot entries write them; out_frames (B)
 *          int32 the frames the utterance has consumed.  A hypothesis is never longer than the frames consumed; with a smaller
 *          Lcap the ids are cut at Lcap, out_len is the full length, and nothing is written out of range.
 * Every kernel that opens the state compares the utterance's header with its arguments (B, beam_width, max_frames, variant): on a
 * mismatch advance leaves that utterance's state alone, and result writes the unused-slot values in every slot and out_frames -1.
 * All accesses stay inside the state_bytes that the arguments name, which are checked against the state_bytes passed.
 * NULL or non-positive arguments: ASR_ERR_BAD_ARG; the limits of asr_ctc_beam_search and max_frames * beam_width beyond int32:
 * ASR_ERR_UNSUPPORTED; a short state or workspace: ASR_ERR_WORKSPACE; the model and graph argument checks of
 * asr_ctc_beam_search_lm and asr_ctc_beam_search_bias.  All checks run before the first launch.  No entry allocates, synchronises
 * or copies to the host: reset, advance and result can be enqueued back to back on one stream.  Bitwise reproducible. */
size_t asr_ctc_beam_stream_state_bytes(int B, int beam_width, int max_frames, int with_lm, int with_bias);
size_t asr_ctc_beam_stream_workspace_bytes(int Tc, int B, int V, int beam_width, int top_k);
int asr_ctc_beam_stream_reset(void* stream, void* state, size_t state_bytes, int B, int beam_width, int max_frames, int with_lm,
                              int with_bias, int bos, const int32_t* mask);
int asr_ctc_beam_stream_advance(void* stream, const float* logits, const int32_t* lengths, int Tc, int B, int V, int blank,
                                int beam_width, int top_k, float min_logp, const float* uni, int vlm, const int32_t* keys,
                                const float* vals, int slots, int max_probe, int order, const int32_t* g_keys, const int32_t* g_vals,
                                int g_slots, int g_max_probe, const float* g_ret, int g_n_states, float alpha, float beta,
                                int frames_before, int max_frames, void* state, size_t state_bytes, void* workspace,
                                size_t workspace_bytes);
int asr_ctc_beam_stream_result(void* stream, const float* uni, int vlm, const int32_t* keys, const float* vals, int slots,
                               int max_probe, int order, const int32_t* g_keys, const int32_t* g_vals, int g_slots, int g_max_probe,
                               const float* g_ret, int g_n_states, float alpha, float beta, int eos, int B, int beam_width,
                               int max_frames, int blank, int Lcap, const void* state, size_t state_bytes, int32_t* out_ids,
                               int32_t* out_len, float* out_score, float* out_ctc, float* out_lm, float* out_bias,
                               int32_t* out_frames);
/* Gram-CTC beam search over spelled strings: asr_ctc_beam_search for an inventory of a blank, unigrams and
 * bigrams spelled by two unigrams (the loss asr_ctc_forward computes with label_bigram).  The hypotheses are strings of unigrams; a
 * string carries the mass of its paths that end in blank, in the unigram token of its last character and in the bigram token of its
 * last two, so every way of cutting it into tokens that the beam kept is summed: out_score is log p(string | x) as far as the beam
 * kept its paths (a lower bound on minus the Gram-CTC loss of the string with every bigram of the table offered).
 *   gram      (V, 2) i32 on the device: (u, -1) a unigram token, (u1, u2) a bigram token, (-1, -1) the blank and any id that is
 *             never emitted (such a candidate is dropped after the top_k / min_logp choice).  No two tokens share a row.
 *   out_ids   (B, beam_width, 2T) unigram ids of the final beam sorted by score descending, padded with blank (a bigram token adds
 *             two characters in one frame)      out_len, out_score (B, beam_width) as asr_ctc_beam_search
 *   workspace asr_gram_ctc_beam_workspace_bytes(T, B, V, beam_width, top_k) bytes
 * Candidates, limits, tie rules and error codes of asr_ctc_beam_search; gram == NULL is ASR_ERR_UNSUPPORTED.  Every element of
 * every output is written on every call; an utterance without frames gives the empty string with score 0 in slot 0.  With a table
 * without bigram rows whose unigram ids are the token ids, the first T columns, out_len and out_score are asr_ctc_beam_search's.
 * Bitwise reproducible. */
size_t asr_gram_ctc_beam_workspace_bytes(int T, int B, int V, int beam_width, int top_k);
int asr_gram_ctc_beam_search(void* stream, const float* logits, const int32_t* lengths, int T, int B, int V, int blank,
                             int beam_width, int top_k, float min_logp, const int32_t* gram, void* workspace, size_t workspace_bytes,
                             int32_t* out_ids, int32_t* out_len, float* out_score);
/* Gram-CTC beam search fused with a character n-gram language model: asr_gram_ctc_beam_search with every
 * string S carrying lm(S) and ranked, in every frame, by  total(S) + (alpha * lm(S) + beta * len(S))  in f32, the expression of
 * asr_ctc_beam_search_lm with len counted in characters.
 * Model: the image above (order 1-4) over the unigram ids that `gram` spells with (the table's values, not the token ids).
 *   vlm >= V as above; <s> / </s> are ids >= V; the unigram entries of bigram-token ids are never queried.
 * lm(S) is a function of the string alone: lm(()) = 0 and lm(S + c) = lm(S) + step(context(S), c) in f32, context(S) the last
 *   order - 1 characters of S, (bos) before them when bos >= 0.  A bigram extension (a, b) adds its two steps in string order,
 *   (lm(S) + step(ctx(S), a)) + step(ctx(S + a), b), so every route to a string (and a string pruned and created again) gives the
 *   same f32 value: the left-to-right sum of its steps.
 * total(S) is the frame's merged Gram-CTC total exactly as asr_gram_ctc_beam_search forms it (the stay plus the absorbed unigram
 *   and bigram extensions; two extensions of one string merged); the bonus is added after the merges, every contributor of a
 *   string having the same lm and len.  Merging, canonical positions, tie rules, dropped (-1, -1) candidates and the prefix table
 *   are those of the unfused entry; the three masses stay pure Gram-CTC quantities.
 * After the last frame, when eos >= 0, lm += step(ctx(S), eos); out_score = out_ctc + (alpha * out_lm + beta * len), and the beam
 *   is ranked again by counting, ties to the earlier slot.
 *   out_ids (B, beam_width, 2T), out_len, out_score (the combined score) as asr_gram_ctc_beam_search
 *   out_ctc (B, beam_width) f32 logaddexp of the three masses, unused -inf       out_lm (B, beam_width) f32 lm(S), unused 0
 *   workspace asr_gram_ctc_beam_lm_workspace_bytes(T, B, V, beam_width, top_k) bytes
 * Every element of every output is written on every call; an utterance without frames gives the empty string in slot 0 with
 * out_ctc 0, out_lm the eos step (0 without eos) and out_score combined accordingly.  With alpha = beta = 0 and eos < 0, out_ids,
 * out_len and out_score equal asr_gram_ctc_beam_search's bit for bit and out_ctc == out_score.  With a table without bigram rows
 * whose unigram ids are the token ids, the first T columns, out_len and the three scores are asr_ctc_beam_search_lm's.
 * Limits and errors are the union of the two parents', all checked before the first launch: beam_width > 128, top_k > 64,
 * beam_width * top_k > 4096, 2 * T * beam_width beyond int32, gram == NULL, order > 4: ASR_ERR_UNSUPPORTED; the model-argument
 * checks of asr_ctc_beam_search_lm (order < 1, slots, max_probe, vlm < V, bos or eos >= vlm): ASR_ERR_BAD_ARG; a short workspace:
 * ASR_ERR_WORKSPACE.  Frames past lengths[b] are never read.  Bitwise reproducible. */
size_t asr_gram_ctc_beam_lm_workspace_bytes(int T, int B, int V, int beam_width, int top_k);
int asr_gram_ctc_beam_search_lm(void* stream, const float* logits, const int32_t* lengths, int T, int B, int V, int blank,
                                int beam_width, int top_k, float min_logp, const int32_t* gram, const float* uni, int vlm,
                                const int32_t* keys, const float* vals, int slots, int max_probe, int order, int bos, int eos,
                                float alpha, float beta, void* workspace, size_t workspace_bytes, int32_t* out_ids,
                                int32_t* out_len, float* out_score, float* out_ctc, float* out_lm);
/* Streaming Gram-CTC beam search: asr_gram_ctc_beam_search or asr_gram_ctc_beam_search_lm fed chunk by
 * chunk, the beam of strings carried between the calls in a device-resident state: the contract of the asr_ctc_beam_stream_*
 * block above.  For every cutting of the frames into chunks, result after a chunk is bit for bit the output of the one-shot entry
 * on the frames so far (its first min(2T, Lcap) id columns).  uni == NULL: no model (the other model arguments are ignored).  The
 * same variant, B, beam_width and max_frames go to every call on one state.
 *   state     asr_gram_ctc_beam_stream_state_bytes(B, beam_width, max_frames, with_lm) bytes, 256-byte aligned.  Per utterance the
 *             header of the CTC stream's state, in the same place, with a Gram bit in its variant word; the beam's per-string
 *             fields as arrays of beam_width entries (pb, pu, pg, the hashes of s, s[:-1], s[:-2], len, the last three
 *             characters, the tokens behind pu and pg, node; with a model lm); and the prefix table of 2 * max_frames * beam_width
 *             (parent node, character) pairs.  Opaque to the caller; copying the bytes copies the search.
 *   workspace asr_gram_ctc_beam_stream_workspace_bytes(Tc, B, V, beam_width, top_k) bytes: the candidate rows of one chunk and
 *             their spellings, per call; it does not depend on beam_width
 * reset:   writes the header and the root beam (the empty string) of every utterance, or, with mask (B) int32, of the utterances
 *          with mask[b] != 0.  It takes no bos: a string's model context is its last characters with (bos) before them, which
 *          advance and result form from the bos they are given; the same bos goes to both.
 * advance: consumes logits (Tc, B, V) f32 with gram (V, 2) as in the one-shot entry; lengths, frames_before, max_frames and the
 *          device-side clamp as in asr_ctc_beam_stream_advance.
 * result:  the end term (with a model and eos >= 0, lm += step(ctx(S), eos)), the final order and the backtrack of the one-shot
 *          entry, applied to the saved beam; the state is not changed.  out_ids (B, beam_width, Lcap) padded with blank; out_len,
 *          out_score (B, beam_width); out_ctc, out_lm with a model (NULL otherwise); out_frames (B) int32 the frames the utterance
 *          has consumed.  A string is never longer than twice the frames consumed; with a smaller Lcap the ids are cut at Lcap,
 *          out_len is the full length, and nothing is written out of range.
 * A header mismatch (B, beam_width, max_frames, variant) is handled as in the CTC stream: advance leaves that utterance's state
 * alone, result writes the unused-slot values in every slot and out_frames -1.  The two families refuse each other's states the
 * same way: a state reset by asr_ctc_beam_stream_reset is a mismatch here, and one reset here is a mismatch there.
 * NULL or non-positive arguments: ASR_ERR_BAD_ARG; gram == NULL, the limits of asr_gram_ctc_beam_search, frames_before + Tc >
 * max_frames and 2 * max_frames * beam_width beyond int32: ASR_ERR_UNSUPPORTED; a short state or workspace: ASR_ERR_WORKSPACE; the
 * model argument checks of asr_gram_ctc_beam_search_lm.  All checks run before the first launch.  No entry allocates, synchronises
 * or copies to the host.  Bitwise reproducible. */
size_t asr_gram_ctc_beam_stream_state_bytes(int B, int beam_width, int max_frames, int with_lm);
size_t asr_gram_ctc_beam_stream_workspace_bytes(int Tc, int B, int V, int beam_width, int top_k);
int asr_gram_ctc_beam_stream_reset(void* stream, void* state, size_t state_bytes, int B, int beam_width, int max_frames, int with_lm,
                                   const int32_t* mask);
int asr_gram_ctc_beam_stream_advance(void* stream, const float* logits, const int32_t* lengths, int Tc, int B, int V, int blank,
                                     int beam_width, int top_k, float min_logp, const int32_t* gram, const float* uni, int vlm,
                                     const int32_t* keys, const float* vals, int slots, int max_probe, int order, int bos,
                                     float alpha, float beta, int frames_before, int max_frames, void* state, size_t state_bytes,
                                     void* workspace, size_t workspace_bytes);
int asr_gram_ctc_beam_stream_result(void* stream, const float* uni, int vlm, const int32_t* keys, const float* vals, int slots,
                                    int max_probe, int order, int bos, int eos, float alpha, float beta, int B, int beam_width,
                                    int max_frames, int blank, int Lcap, const void* state, size_t state_bytes, int32_t* out_ids,
                                    int32_t* out_len, float* out_score, float* out_ctc, float* out_lm, int32_t* out_frames);
/* Gram-CTC beam search with contextual phrase biasing: asr_gram_ctc_beam_search_lm (uni != NULL) or
 * asr_gram_ctc_beam_search (uni == NULL: the other model arguments are ignored and out_lm is all 0) with the automaton of the
 * asr_ctx_score block above running beside every string.
 * Graph: that image over the unigram ids that `gram` spells with (the table's values, not the token ids), as the model of
 *   asr_gram_ctc_beam_search_lm; the caller builds it with V the logits' V and the logits' blank.  A phrase that contains an id which
 *   no row of gram spells can never match; that is allowed.
 * bias_open(S) and state(S) are functions of the string alone: state(()) is the root, bias_open(()) = 0, and
 *   bias_open(S + c) = bias_open(S) + delta(state(S), c)  in f32 with the look-up stated above (hit at (s, c); else hit at (0, c)
 *   paying ret[s] + delta0; else the root paying ret[s]; a next outside [0, n_states) counts as the root).  A bigram extension (a, b)
 *   takes two dependent steps in string order, (bias_open(S) + delta(s, a)) + delta(s1, b) with s1 the state after a, so every route
 *   to a string (and a string pruned and created again) gives the same f32 value and the same state.
 * Ranking, in every frame and after all merges of the frame:  (total + (alpha * lm + beta * len)) + bias_open  resp.
 *   total + bias_open  in f32, total, lm and len as in asr_gram_ctc_beam_search_lm.  Merging (two extensions of one string; a stay
 *   with the extensions that spell it), canonical positions, tie rules, dropped (-1, -1) candidates and the prefix table are the
 *   parents'; a merged entry keeps the stay's values; pb / pu / pg stay pure Gram-CTC quantities.
 * After the last frame bias(S) = bias_open(S) + ret[state(S)], the sum of weight * length over every occurrence of every phrase in
 *   S; the eos term goes into lm as in the parent; the beam is sorted by  out_score = (out_ctc + (alpha * out_lm + beta * len)) +
 *   out_bias  resp.  out_ctc + out_bias,  ties to the earlier slot.
 *   out_ids (B, beam_width, 2T), out_len, out_score, out_ctc, out_lm as asr_gram_ctc_beam_search_lm
 *   out_bias (B, beam_width) f32 bias(S), unused 0
 *   workspace asr_gram_ctc_beam_bias_workspace_bytes(T, B, V, beam_width, top_k) bytes
 * Every element of every output is written on every call.  With a graph without phrases (n_states 1, slots 0) the outputs equal the
 * parent entry's bit for bit and out_bias is all 0.  With a table without bigram rows whose unigram ids are the token ids, the first
 * T columns, out_len and the four scores are asr_ctc_beam_search_bias's.  Errors are the union of the parents', all checked before
 * the first launch: the limits and model checks of asr_gram_ctc_beam_search_lm (gram == NULL: ASR_ERR_UNSUPPORTED) and the
 * graph-argument checks of asr_ctc_beam_search_bias (ASR_ERR_BAD_ARG; NULL out_ctc, out_lm or out_bias too).  Frames past
 * lengths[b] are never read.  No host synchronisation.  Bitwise reproducible.
 * Streaming: the asr_gram_ctc_beam_stream_* contract with a graph.  advance and result take the six graph arguments after bos
 * resp. eos; g_ret == NULL: no graph (the other graph arguments must then be NULL / 0).  result also takes out_bias (with a graph;
 * NULL otherwise), and out_ctc / out_lm are written with a model or a graph.  The per-call workspace is
 * asr_gram_ctc_beam_stream_workspace_bytes.  With with_bias == 0 the size, the header's variant word and every byte of the state
 * are those of the asr_gram_ctc_beam_stream_* entries, and a state can move between the two families.  With a graph the variant word
 * gains a bias bit and the state gains bias_open and the automaton state per string, beside lm.  A variant mismatch (a state reset
 * without the bias bit given to a call with a graph, or the reverse; a CTC stream's state) is handled as there: advance leaves the
 * utterance alone, result writes the unused-slot values and out_frames -1.  Error codes: those of asr_gram_ctc_beam_stream_* and
 * the graph-argument checks above. */
size_t asr_gram_ctc_beam_bias_workspace_bytes(int T, int B, int V, int beam_width, int top_k);
int asr_gram_ctc_beam_search_bias(void* stream, const float* logits, const int32_t* lengths, int T, int B, int V, int blank,
                                  int beam_width, int top_k, float min_logp, const int32_t* gram, const float* uni, int vlm,
                                  const int32_t* keys, const float* vals, int slots, int max_probe, int order, int bos, int eos,
                                  float alpha, float beta, void* workspace, size_t workspace_bytes, int32_t* out_ids,
                                  int32_t* out_len, float* out_score, float* out_ctc, float* out_lm, const int32_t* g_keys,
                                  const int32_t* g_vals, int g_slots, int g_max_probe, const float* g_ret, int g_n_states,
                                  float* out_bias);
size_t asr_gram_ctc_beam_bias_stream_state_bytes(int B, int beam_width, int max_frames, int with_lm, int with_bias);
int asr_gram_ctc_beam_bias_stream_reset(void* stream, void* state, size_t state_bytes, int B, int beam_width, int max_frames,
                                        int with_lm, int with_bias, const int32_t* mask);
int asr_gram_ctc_beam_bias_stream_advance(void* stream, const float* logits, const int32_t* lengths, int Tc, int B, int V, int blank,
                                          int beam_width, int top_k, float min_logp, const int32_t* gram, const float* uni, int vlm,
                                          const int32_t* keys, const float* vals, int slots, int max_probe, int order, int bos,
                                          const int32_t* g_keys, const int32_t* g_vals, int g_slots, int g_max_probe,
                                          const float* g_ret, int g_n_states, float alpha, float beta, int frames_before,
                                          int max_frames, void* state, size_t state_bytes, void* workspace, size_t workspace_bytes);
int asr_gram_ctc_beam_bias_stream_result(void* stream, const float* uni, int vlm, const int32_t* keys, const float* vals, int slots,
                                         int max_probe, int order, int bos, int eos, const int32_t* g_keys, const int32_t* g_vals,
                                         int g_slots, int g_max_probe, const float* g_ret, int g_n_states, float alpha, float beta,
                                         int B, int beam_width, int max_frames, int blank, int Lcap, const void* state,
                                         size_t state_bytes, int32_t* out_ids, int32_t* out_len, float* out_score, float* out_ctc,
                                         float* out_lm, float* out_bias, int32_t* out_frames);
/* Commit: streams of any length.  The prefix table of a stream holds max_frames rows and advance never frees
 * one; a commit makes a prefix of the hypotheses final, drops the hypotheses that disagree with it, and rewrites the table so that
 * it holds only what comes after that prefix.  A caller that commits "the best hypothesis minus its last few tokens" every few
 * chunks feeds a stream of any length through a table of a few dozen rows.  Both families, every variant; per_frame below is 1 for
 * the CTC stream and 2 for the Gram-CTC stream (a token there is a character).
 *   Every utterance has a committed count c: header word 7 of its state, 0 after reset.  Every live hypothesis has len tokens, and
 *   its first c are the committed ones.  commit(P), P a string of n >= 0 tokens per utterance (prefix_ids (B, prefix_pitch),
 *   prefix_len (B)), does per utterance:
 *   prune    exactly the hypotheses whose tokens [c, c + n) equal P are kept.
 *   refuse   if none would be kept, if n > prefix_pitch, or if the kept tails need more than min(max_rows, max_frames) rows, the
 *            utterance's state is left as it is and status is 0.
 *   beam     the kept entries move to the front of every per-slot array in their order (the searches rank ties to the lower slot,
 *            so the order is part of the search state) and the occupancy becomes their number.  len, the hashes, the model
 *            contexts and the automaton states stay absolute: every score and every later ranking has the bits it would have
 *            had.  The slots the beam leaves behind get 0.
 *   compact  the tail of kept slot i is its l_i = len[i] - c - n tokens after P; tail position j becomes node j * beam_width + i
 *            with parent (j - 1) * beam_width + i (-1 for j = 0), node[i] = (l_i - 1) * beam_width + i or -1, and the rest of
 *            the rows that were in use gets 0.  The header's frames word becomes rows = ceil(max_i l_i / per_frame), and the next
 *            advance allocates from that row on.  So after the first commit that word means "table rows in use" (it is what
 *            result's out_frames reports and what advance's frames_before must bound); for a stream that never committed it
 *            equals the frames consumed.  c += n.
 *   auto     prefix_len[b] < 0, or prefix_ids == NULL for every utterance: P is the longest common prefix of all live hypotheses
 *            beyond c.  Nothing is pruned, and whatever the stream returns afterwards is, after prepending the committed tokens,
 *            bit for bit what it would have returned without the call.
 *   compact == 0 makes the call read-only: the outputs say what it would commit, the state is not written.
 * Outputs per utterance: out_status 1 applied, 0 refused, -1 header mismatch (the state is left alone, out_committed and out_rows
 * are -1); out_ids (B, out_pitch) the first min(n, out_pitch) tokens this call committed (the rest of a row is not written), out_len
 * their count n (0 unless applied); out_committed the new c; out_rows the rows in use after the call.
 * After a commit, result returns tails: out_ids holds the tokens after the c committed ones and out_len = len - c; the scores are
 * those of the whole hypotheses.  With c = 0 this is the result described above.
 *   workspace asr_beam_stream_commit_workspace_bytes(B, beam_width, max_frames, per_frame) bytes: the live tails, staged
 * Errors as in the other streaming entries (NULL state, workspace or output, out_pitch <= 0, max_rows < 0, prefix_ids without
 * prefix_len or with prefix_pitch <= 0: ASR_ERR_BAD_ARG; then the limits: ASR_ERR_UNSUPPORTED; a short state or workspace:
 * ASR_ERR_WORKSPACE), all before the launch.  One launch, no atomics, nothing allocated, copied to the host or synchronised; the
 * same inputs give the same state bytes.  The Gram-CTC entry's state is that of asr_gram_ctc_beam_bias_stream_state_bytes. */
size_t asr_beam_stream_commit_workspace_bytes(int B, int beam_width, int max_frames, int per_frame);
int asr_ctc_beam_stream_commit(void* stream, void* state, size_t state_bytes, int B, int beam_width, int max_frames, int with_lm,
                               int with_bias, const int32_t* prefix_ids, int prefix_pitch, const int32_t* prefix_len, int compact,
                               int max_rows, void* workspace, size_t workspace_bytes, int32_t* out_ids, int out_pitch,
                               int32_t* out_len, int32_t* out_committed, int32_t* out_rows, int32_t* out_status);
int asr_gram_ctc_beam_stream_commit(void* stream, void* state, size_t state_bytes, int B, int beam_width, int max_frames, int with_lm,
                                    int with_bias, const int32_t* prefix_ids, int prefix_pitch, const int32_t* prefix_len,
                                    int compact, int max_rows, void* workspace, size_t workspace_bytes, int32_t* out_ids,
                                    int out_pitch, int32_t* out_len, int32_t* out_committed, int32_t* out_rows,
                                    int32_t* out_status);

/* ---------------------------------------------------------------------------------------- dense projections
 * bf16 MFMA GEMMs (f32 accumulate).  Replace the BLAS/cuDNN calls behind chainer.links.Linear, the 1x1
 * ConvolutionND of asr/nn/convolution_1d.py:7-38, the SRU projection asr/nn/sru.py:340-341,421-429 and -- through
 * asr_im2col / asr_col2im -- chainer.links.Convolution2D (asr/nn/nn.py:235-238).
 *   asr_gemm_nt      C[M,N] = A[M,K] * B[N,K]^T (+ bias[N]);  A, B bf16, k-contiguous (fast path: lda/ldb/K multiples
 *                    of 8 and 16-byte aligned bases; anything else takes element loads); C f32 (out_bf16 = 0) or bf16 (1)
 *   asr_gemm_tn_acc  C[M,N] += A[K,M]^T * B[K,N];  A, B bf16 row-major; C f32, accumulated with atomics (split-K)
 *   asr_gemm_tn_acc_group  n <= 4 such products (any shapes) in ONE launch; every argument a host array of n entries:
 *                    the weight gradients a recurrence releases together (dW_ih and the per-direction dW_hh of
 *                    chainer.links.NStepBiGRU, asr/nn/nn.py:3 -- cuDNN's RNN backward-weights forms them in one call too).
 *                    Two products may add into the same output.
 */
int asr_gemm_nt(void* stream, const void* A, int lda, const void* B, int ldb, void* C, int ldc, const float* bias,
                int M, int N, int K, int out_bf16);
/* asr_gemm_nt_8ph: the same product (no element-load fall-back: K % 8 == 0, N % 4 == 0, lda / ldb multiples of 8, ldc of 4, 16-byte aligned
 * bases, operands below 2 GiB -- asr_gemm_nt_8ph_ok says whether a call qualifies) on the 256 x 256 tile kernel with eight waves in
 * two staggered groups (csrc/gemm8.hip); asr_gemm_nt routes the model's products to it.  With more than 256 tiles and K % 64 == 0,
 * 128 <= K <= 1024 (N <= 8192; bf16 output: N and ldc multiples of 8) it runs as ONE persistent workgroup per CU that walks its tiles as one
 * stream of K steps (gemm_nt_8pp_kernel): the forward projections of a recurrent layer (chainer.links.NStepBiGRU's W x, asr/nn/nn.py:3). */
int asr_gemm_nt_8ph_ok(const void* A, int lda, const void* B, int ldb, const void* C, int ldc, const float* bias, int M, int N, int K,
                       int out_bf16);
int asr_gemm_nt_8ph(void* stream, const void* A, int lda, const void* B, int ldb, void* C, int ldc, const float* bias, int M, int N, int K,
                    int out_bf16);
int asr_gemm_tn_acc(void* stream, const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N, int K);
int asr_gemm_tn_acc_group(void* stream, int n, const void* const* A, const int* lda, const void* const* B, const int* ldb,
                          float* const* C, const int* ldc, const int* M, const int* N, const int* K);
/* asr_gemm_tn_acc_group_8ph: the same products on the 256 x 256 tile / eight-wave kernel of csrc/gemm8.hip (transposing LDS reads);
 * every product must pass asr_gemm_tn_8ph_ok (M, N, lda, ldb multiples of 8, 16-byte aligned bases, operands below 2 GiB).
 * asr_gemm_tn_acc / asr_gemm_tn_acc_group route qualifying calls to it. */
int asr_gemm_tn_8ph_ok(const void* A, int lda, const void* B, int ldb, const float* C, int ldc, int M, int N, int K);
int asr_gemm_tn_acc_group_8ph(void* stream, int n, const void* const* A, const int* lda, const void* const* B, const int* ldb,
                              float* const* C, const int* ldc, const int* M, const int* N, const int* K);

/* ---------------------------------------------------------------------------------------- layout / activations
 * Internal activations are (T, B, H, C) bf16 (time-major, channel-last); see DESIGN.md "Data layout in HBM".
 *   asr_cast_bf16     f32 (rows, cols) -> bf16, optionally transposed to (cols, rows)    [weight copies]
 *   asr_cast_bf16_many  the same for a table of matrices in one launch: jobs_dev = njobs x 6 long long in device
 *                     memory {src, dst, rows, cols, transpose, first_tile}; a tile is 64x64 elements of src, tiles are
 *                     numbered job after job, total_tiles = their sum  [all weight copies after an optimiser step]
 *   asr_permute4      dense dst (d0,d1,d2,d3) <- strided src (element strides s0..s3), f32/bf16 either side
 *   asr_im2col        col[(t,b,ho)][(kh,kw,ci)] (row pitch Kp, zero padded) from x with element strides
 *                     (sT,sB,sH,sC); reads x[t+kw-pad_t, b, ho+kh-pad_h, ci] for t in [0, Tout).  pad_t = KW-1 with
 *                     Tout = T + KW-1 is the reference's conv (pad both sides), Tout = T its causal crop
 *                     x[..., :-pad] (run/ctc/cnn/model.py:43-44)
 *   asr_col2im        adjoint of asr_im2col for a (T,B,Hin,Cin) bf16 input gradient
 *   asr_maxout2_*     nn.Maxout(2): asr/nn/nn.py:45-50 (pairs of adjacent channels; ties -> first)
 *   asr_maxpool_h_*   nn.MaxPooling2D(ksize=(k,1)): asr/nn/nn.py:95-103, stride k, cover_all=True
 *   asr_add_bf16      residual add (asr/nn/nn.py:322-328)
 *   asr_colsum_acc    out[c] += sum_r x[r][c]   (bias gradients)
 */
int asr_cast_bf16(void* stream, const float* src, void* dst, int rows, int cols, int transpose);
int asr_cast_bf16_many(void* stream, const long long* jobs_dev, int njobs, long long total_tiles);
int asr_bf16_to_f32(void* stream, const void* src, float* dst, long long n);
int asr_permute4(void* stream, const void* src, int src_bf16, void* dst, int dst_bf16, int d0, int d1, int d2, int d3,
                 long long s0, long long s1, long long s2, long long s3);
int asr_im2col(void* stream, const void* x, int x_bf16, long long sT, long long sB, long long sH, long long sC, int T,
               int B, int Hin, int Cin, int KH, int KW, int pad_h, int pad_t, int Tout, int Kp, void* col);
int asr_col2im(void* stream, const void* dcol, int T, int B, int Hin, int Cin, int KH, int KW, int pad_h, int pad_t,
               int Tout, int Kp, void* dx);
/* Convolution2D weights (Co, Ci, kh, kw) f32 <-> the GEMM's (Co, Kp) matrix with k = (kh, kw, ci) */
int asr_conv_weight_pack(void* stream, const float* W, void* dst_bf16, int Co, int Ci, int KH, int KW, int Kp,
                         int transpose);
/* implicit-GEMM convolution (no column matrix): x (Ts, B, Hs, Cs) bf16 with Cs % 8 == 0; W rows of pitch ldw >= KH*KW*Cs,
 * ldw % 32 == 0 and ldw % Cs == 0 (columns behind KH*KW*Cs are empty taps and must hold zeros);
 * out[(t, b, h)][n] = sum_{kh,kw,c} x[t + sgn (kw - pad_t)][b][h + sgn (kh - pad_h)][c] * W[n][(kh*KW + kw)*Cs + c]  (+ bias)
 * over rows t < Tr, h < Hr (zero outside x).  sgn = +1, rows = output positions, W = asr_conv_weight_pack(.., 0): the
 * forward convolution of nn.Convolution2D (asr/nn/nn.py:235-238); sgn = -1, x = output gradient, rows = input positions,
 * W = asr_conv_weight_pack_bwd: its backward-data.  out (Tr*B*Hr, N) bf16 or f32.
 * asr_conv_weight_pack_bwd: dst[ci][(kh*KW + kw)*Co + co] = W[co][ci][kh][kw] as bf16. */
int asr_conv_nt(void* stream, const void* x, const void* W, int ldw, void* out, int out_bf16, const float* bias, int Ts, int B,
                int Hs, int Cs, int KH, int KW, int pad_h, int pad_t, int sgn, int Tr, int Hr, int N);
/* asr_conv_nt_8ph: the same implicit convolution on the eight-wave kernel of csrc/gemm8.hip (Cs and the row pitch of W multiples of 64,
 * N % 4 == 0, Hs < 256, 16-byte aligned operands: asr_conv_nt_8ph_ok); asr_conv_nt routes the products with more than 128 output
 * columns that the LDS-resident kernel does not take to it. */
int asr_conv_nt_8ph_ok(const void* x, const void* W, int ldw, const void* out, int out_bf16, const float* bias, int Ts, int B, int Hs, int Cs,
                       int KH, int KW, int Tr, int Hr, int N);
int asr_conv_nt_8ph(void* stream, const void* x, const void* W, int ldw, void* out, int out_bf16, const float* bias, int Ts, int B, int Hs,
                    int Cs, int KH, int KW, int pad_h, int pad_t, int sgn, int Tr, int Hr, int N);
/* asr_conv_nt_8pn: the narrow form (N <= 128 output columns: 256 x 64 / 256 x 128 tiles) of the same kernel family */
int asr_conv_nt_8pn_ok(const void* x, const void* W, int ldw, const void* out, int out_bf16, const float* bias, int Ts, int B, int Hs, int Cs,
                       int KH, int KW, int Tr, int Hr, int N);
int asr_conv_nt_8pn(void* stream, const void* x, const void* W, int ldw, void* out, int out_bf16, const float* bias, int Ts, int B, int Hs,
                    int Cs, int KH, int KW, int pad_h, int pad_t, int sgn, int Tr, int Hr, int N);
/* The same product with the activation block of a tile resident in LDS (csrc/conv_direct.hip): one workgroup = one utterance x 256 / Hr
 * time steps x all Hr heights x 64 or 128 output columns; the (Tt + KW - 1) x (Hr + KH - 1) x Cs activations it can touch are loaded
 * once instead of once per tap.  bf16 output, Cs in {32, 64, 128, 256}, ldw % 32 == 0; asr_conv_direct_ok says whether a shape is
 * served (asr_conv_nt asks and dispatches by itself; ASR_DEBUG conv_direct=0 keeps the implicit-GEMM kernels). */
int asr_conv_direct_ok(int Ts, int B, int Hs, int Cs, int KH, int KW, int Tr, int Hr, int N, int K, int out_bf16);
int asr_conv_direct_nt(void* stream, const void* x, const void* W, int ldw, void* out, const float* bias, int Ts, int B, int Hs, int Cs,
                       int KH, int KW, int pad_h, int pad_t, int sgn, int Tr, int Hr, int N);
/* The first block of the models -- Convolution2D over the 8-channel padded features, Maxout(2), MaxPooling2D((k, 1)) (asr/nn/nn.py:235-238,
 * :45-50, :95-103 as run/ctc/cnn/model.py:42-48 stacks them) -- as ONE forward and ONE backward pass (csrc/conv_first.hip): the convolution
 * output (311 MB at T=1000, B=32 for BASELINE configs[1]) and its gradient never exist.
 * asr_conv_mp_ok: 1 <= Ci <= 8 real input channels, KH KW <= 15 taps, Co % 128 == 0, 2 <= k <= 4.
 * asr_conv_mp_fwd: x8 (Ts, B, Hs, 8) bf16 (asr_pack_input_pad); W (Co, 128) bf16, k = (kh KW + kw) 8 + ci, zeros behind 8 KH KW
 *   (asr_conv_weight_pack with Kp = 128); bias (Co) f32 or NULL; y (Tout, B, Hp, Co / 2) bf16 with Hp = cover_all pooled heights of Hout;
 *   idx (same shape, bytes): 2 * (row of the window) + (second channel of the pair) of the winner.  Values and tie rules of asr_conv_nt
 *   (bf16 out) followed by asr_maxout2_pool_fwd.
 * asr_conv_mp_bwd: gy (Tout, B, Hp, Co / 2) bf16, idx and x8 of the forward call; gW (Co, Ci, KH, KW) f32 += the weight gradient,
 *   gb (Co) f32 += the bias gradient (NULL: none); workspace: asr_conv_mp_bwd_workspace(Tout, B, Hout, Co, k) bytes, 16-byte aligned. */
int asr_conv_mp_ok(int Ci, int KH, int KW, int Co, int k);
int asr_conv_mp_fwd(void* stream, const void* x8, const void* W, int ldw, const float* bias, void* y, void* idx, int Ts, int B, int Hs,
                    int KH, int KW, int pad_h, int pad_t, int Tout, int Hout, int Co, int k);
long long asr_conv_mp_bwd_workspace(int Tout, int B, int Hout, int Co, int k);
int asr_conv_mp_bwd(void* stream, const void* gy, const void* idx, const void* x8, void* workspace, float* gW, float* gb, int Ts, int B,
                    int Hs, int Ci, int KH, int KW, int pad_h, int pad_t, int Tout, int Hout, int Co, int k);
/* any strided (T, B, H, C) f32 / bf16 tensor -> dense (T, B, H, Cpad) bf16, channels C..Cpad-1 zero: brings the loader's
 * (B, 3, 40, T) float32 minibatch into the layout of asr_conv_nt (first layer: C = 3 -> Cpad = 8) */
int asr_pack_input_pad(void* stream, const void* x, int x_bf16, long long sT, long long sB, long long sH, long long sC, int T,
                       int B, int H, int C, int Cpad, void* out_bf16);
int asr_conv_weight_pack_bwd(void* stream, const float* W, void* dst, int Co, int Ci, int KH, int KW);
/* weight gradient of the same convolution without a column matrix: g (Tr*B*Hr, Co) bf16 rows of pitch ldg = output gradient,
 * C[co][(kh*KW + kw)*Cs + c] += sum_{t,b,h} g[(t, b, h)][co] * x[t + kw - pad_t][b][h + kh - pad_h][c]   (f32, split-K atomics);
 * Cs % 8 == 0.  asr_conv_weight_grad_unpack adds such a (Co, Kp) scratch into the (Co, Ci, KH, KW) gradient; Cs = channel
 * pitch of the scratch rows (>= Ci; 0 = Ci). */
int asr_conv_tn_acc(void* stream, const void* g, int ldg, const void* x, float* C, int ldc, int Co, int Ts, int B, int Hs,
                    int Cs, int KH, int KW, int pad_h, int pad_t, int Tr, int Hr);
/* asr_conv_tn_acc_8ph: the same weight gradient on the eight-wave kernel of csrc/gemm8.hip (Co, Cs, ldg multiples of 8, 16-byte aligned
 * operands: asr_conv_tn_8ph_ok); asr_conv_tn_acc routes qualifying calls with at least 256 x 256 outputs to it. */
int asr_conv_tn_8ph_ok(const void* g, int ldg, const void* x, const float* C, int ldc, int Co, int Ts, int B, int Hs, int Cs, int KH, int KW,
                       int Tr, int Hr);
int asr_conv_tn_acc_8ph(void* stream, const void* g, int ldg, const void* x, float* C, int ldc, int Co, int Ts, int B, int Hs, int Cs, int KH,
                        int KW, int pad_h, int pad_t, int Tr, int Hr);
int asr_conv_weight_grad_unpack(void* stream, const float* scratch, float* gW, int Co, int Ci, int KH, int KW, int Kp, int Cs);
/* Few output tiles -> hundreds of K splits adding into the same few KB (first layer: 91 of 166 us were the atomics): with
 * asr_conv_tn_copies(...) == 8 the caller hands a zeroed scratch of 8 x (Co, ldc) floats, every XCD adds into its own copy, and
 * asr_conv_weight_grad_unpack_copies sums them into the gradient. */
int asr_conv_tn_copies(int Co, int Cs, int KH, int KW);
int asr_conv_tn_acc_copies(void* stream, const void* g, int ldg, const void* x, float* C, int ldc, int copies, int Co, int Ts, int B,
                           int Hs, int Cs, int KH, int KW, int pad_h, int pad_t, int Tr, int Hr);
int asr_conv_weight_grad_unpack_copies(void* stream, const float* scratch, int copies, float* gW, int Co, int Ci, int KH, int KW, int Kp,
                                       int Cs);
int asr_maxout2_fwd(void* stream, const void* x, void* y, long long n_out);
int asr_maxout2_bwd(void* stream, const void* x, const void* dy, void* dx, long long n_out);
/* Maxout(2) + MaxPooling2D((k, 1)) in one pass: x (R, Hin, 2C) bf16 -> y (R, ceil(Hin / k), C); C % 8 == 0 (else
 * ASR_ERR_UNSUPPORTED: use the two calls).  Same results and tie rules as asr_maxout2_* followed by asr_maxpool_h_*. */
int asr_maxout2_pool_fwd(void* stream, const void* x, void* y, long long R, int Hin, int C, int k);
int asr_maxout2_pool_bwd(void* stream, const void* x, const void* dy, void* dx, long long R, int Hin, int C, int k);
/* The same with the bias gradient of the convolution in front: db (2 C floats, accumulated; may be NULL) += column sums of dx, formed
 * from dy and the winners while both are in registers (replaces the chainer Convolution2D backward's gy.sum over (N, H, W),
 * asr/nn/convolution_2d.py:76-90 through chainer.functions.convolution_2d).  asr_maxout2_pool_bwd_db_ok(C): 1 if db may be given. */
int asr_maxout2_pool_bwd_db(void* stream, const void* x, const void* dy, void* dx, float* db, long long R, int Hin, int C, int k);
int asr_maxout2_pool_bwd_db_ok(int C);
int asr_maxpool_h_fwd(void* stream, const void* x, void* y, long long R, int Hin, int C, int k);
int asr_maxpool_h_bwd(void* stream, const void* x, const void* dy, void* dx, long long R, int Hin, int C, int k);
int asr_add_bf16(void* stream, const void* a, const void* b, void* y, long long n);
/* activations of asr/nn/nn.py:11-73 on bf16: kind 0 relu, 1 clipped_relu(alpha=z), 2 leaky_relu(alpha=slope),
 * 3 elu(alpha), 4 sigmoid, 5 tanh, 6 hard_sigmoid, 7 softplus(alpha=beta); GLU asr/nn/nn.py:267-281 on rows [A|B];
 * dropout (asr/nn/nn.py:211-218) with a counter-based mask that backward regenerates from the same seed. */
int asr_activation_fwd(void* stream, const void* x, void* y, long long n, int kind, float alpha);
int asr_activation_bwd(void* stream, const void* x, const void* dy, void* dx, long long n, int kind, float alpha);
int asr_glu_fwd(void* stream, const void* x, void* y, long long rows, int C);
int asr_glu_bwd(void* stream, const void* x, const void* dy, void* dx, long long rows, int C);
int asr_dropout(void* stream, const void* x, void* y, long long n, float ratio, unsigned int seed);
int asr_colsum_acc(void* stream, const void* x, int x_bf16, long long rows, int cols, int ld, float* out);

/* ---------------------------------------------------------------------------------------- layer normalisation
 * nn.LayerNormalization (asr/nn/nn.py:240-265) = NormalizeLayer (asr/nn/layernorm.py:29-64) + scale/bias on axis 1.
 * rows = T*B, D = H*C contiguous per row, channel = index % C.  No epsilon (the reference ignores it).
 */
int asr_layernorm_fwd(void* stream, const void* x, int x_bf16, void* y, int y_bf16, const float* gamma,
                      const float* beta, float* mean, float* rstd, long long rows, int D, int C);
/* float32 rows normalised over their whole width (C == D, D % 4 == 0, D <= 4096: the logits of a frame over the vocabulary,
 * asr/nn/layernorm.py:33-48 as used by run/ctc/model.py on the output layer): one wave per row, the row in registers, and --
 * lse != NULL -- the log-sum-exp of every output row for asr_ctc_forward_lse.  asr_layernorm_fwd_lse_ok(D, C): 1 if it applies. */
int asr_layernorm_fwd_lse(void* stream, const float* x, float* y, const float* gamma, const float* beta, float* mean, float* rstd,
                          float* lse, long long rows, int D);
int asr_layernorm_fwd_lse_ok(int D, int C);
int asr_layernorm_bwd(void* stream, const void* x, int x_bf16, const void* dy, int dy_bf16, const float* gamma,
                      const float* mean, const float* rstd, void* dx, int dx_bf16, float* dgamma, float* dbeta,
                      long long rows, int D, int C);
/* one-sweep backward of the float32 logits normalisation (x and dy float32, D % 4 == 0, C % 4 == 0, D <= 4096; other
 * shapes: ASR_ERR_UNSUPPORTED, use asr_layernorm_bwd): dx (bf16 or f32, may be NULL) and dgamma += / dbeta += (both or
 * neither) in one pass over x and dy; ws: asr_layernorm_bwd_rows_ws_bytes(rows, D) bytes of scratch for the per-workgroup
 * column sums (0 = shape not supported).  Same formulas as asr_layernorm_bwd (asr/nn/layernorm.py:50-61). */
long long asr_layernorm_bwd_rows_ws_bytes(long long rows, int D);
int asr_layernorm_bwd_rows(void* stream, const float* x, const float* dy, const float* gamma, const float* mean,
                           const float* rstd, void* dx, int dx_bf16, float* dgamma, float* dbeta, long long rows, int D,
                           int C, void* ws, long long ws_bytes);

/* weight normalisation of asr/nn/convolution_2d.py: W = g V / (||V|| + 1e-9) per output channel (:21-25,62-64), its
 * gradient (:92-93, accumulated into gV / gg), and the data-dependent initialisation g = 1/std_t, b = -mean_t/std_t
 * from the first batch's g=1 output (:152-167,177-187). */
int asr_weightnorm_fwd(void* stream, const float* V, const float* g, float* W, float* norm, int Co, int K);
int asr_weightnorm_bwd(void* stream, const float* gW, const float* V, const float* g, const float* norm, float* gV,
                       float* gg, int Co, int K);
int asr_channel_stats(void* stream, const float* x, long long rows, int C, float* mean, float* stdv);
int asr_channel_affine(void* stream, const float* x, const float* scale, const float* shift, void* y_bf16, long long n,
                       int C);
int asr_weightnorm_init(void* stream, const float* mean, const float* stdv, float* g, float* b, int C);

/* dgamma / dbeta += column sums of partial (G, 2, D) written by a one-sweep backward (channel = index % C); with `extra`
 * the buffer is (G, 3, D) and extra[D] += the column sums of the third plane */
int asr_layernorm_fold_partials(void* stream, const float* partial, int G, int D, int C, float* dgamma, float* dbeta, float* extra);
/* Backward of [LayerNormalization over the vocabulary of each frame] -> [one or two CTC-family losses] in one sweep: the
 * gradient with respect to the normalised logits, (softmax - occupancy) * scale * gy summed over the losses
 * (asr/loss/gram_ctc.py:284-297), is formed in registers from the pre-normalisation rows x (T*B, V) f32, the row
 * statistics of asr_layernorm_fwd and the workspaces asr_ctc_forward left behind (ctc_ws: same T, B, Lmax, gram as that
 * call; x_len / gy / gy_per_utt / scale as for asr_ctc_backward), and goes straight into the layer-norm backward
 * (asr/nn/layernorm.py:50-61): dx (f32 or bf16, may be NULL) and dgamma / dbeta ACCUMULATED (both or neither).  V % 4 == 0,
 * V <= 4096, 3*Lmax+1 <= 512.  ws: asr_layernorm_ctc_bwd_ws_bytes(T, B, V) bytes.  dxsum (V floats, or NULL; needs dgamma / dbeta):
 * ACCUMULATES the column sums of dx -- the bias gradient of the projection that produced x. */
long long asr_layernorm_ctc_bwd_ws_bytes(int T, int B, int V);
int asr_layernorm_ctc_bwd(void* stream, const float* x, const float* gamma, const float* beta, const float* mean,
                          const float* rstd, void* dx, int dx_bf16, float* dgamma, float* dbeta, int T, int B, int V, void* ws,
                          long long ws_bytes, int nloss, const void* ctc_ws0, int Lmax0, int gram0, const int32_t* x_len0,
                          const float* gy0, int gy_per_utt0, float scale0, const void* ctc_ws1, int Lmax1, int gram1,
                          const int32_t* x_len1, const float* gy1, int gy_per_utt1, float scale1, float* dxsum);

/* ---------------------------------------------------------------------------------------- batch normalisation
 * chainer.links.BatchNormalization reaches the reference API through `from chainer.links import *` (asr/nn/nn.py:3);
 * Chainer's rule: normalise with the biased batch variance, eps = 2e-5, running averages with decay 0.9 and the
 * unbiased variance.  x, gy, y, dx: (R, C) bf16, channel last (R = every other axis).  ws2C: 2*C doubles of scratch.
 *   asr_batchnorm_stats  mean, rstd = 1/sqrt(var + eps) (C) f32; avg_mean / avg_var (both or neither) updated in place
 *   asr_batchnorm_fwd    y = gamma (x - mean) rstd + beta   (also the inference form, with rstd from the running variance)
 *   asr_batchnorm_bwd    dx (may be NULL) and dgamma / dbeta ACCUMULATED (may be NULL)
 */
int asr_batchnorm_stats(void* stream, const void* x_bf16, long long R, int C, float eps, float decay, double* ws2C,
                        float* mean, float* rstd, float* avg_mean, float* avg_var);
/* out[i] = 1 / sqrt(var[i] + eps): rstd of the inference form from the running variance */
int asr_rsqrt_eps(void* stream, const float* var, float eps, float* out, int n);
int asr_batchnorm_fwd(void* stream, const void* x_bf16, const float* mean, const float* rstd, const float* gamma,
                      const float* beta, long long R, int C, void* y_bf16);
int asr_batchnorm_bwd(void* stream, const void* x_bf16, const void* gy_bf16, const float* mean, const float* rstd,
                      const float* gamma, long long R, int C, double* ws2C, void* dx_bf16, float* dgamma_acc,
                      float* dbeta_acc);

/* ---------------------------------------------------------------------------------------- (Bi)GRU recurrence
 * nn.GRU / nn.NStepBiGRU reach the reference API through `from chainer.links import *` (asr/nn/nn.py:3); gate
 * convention = cuDNN / torch.nn.GRU (r, z, n).  Layouts in csrc/gru.hip.  gi comes from asr_gemm_nt.
 * db_ih / db_hh (ndir, 3H) f32 or NULL: bias gradients, ACCUMULATED (sum over all rows of dgi / dgh).
 * sync_ws: asr_gru_sync_bytes(B, H, ndir) bytes of device memory (control words + the in-launch exchange
 * buffer, zeroed by the call) enabling the persistent
 * one-launch-per-layer form.  mode: 0 = automatic: persistent; a batch of more than 32 utterances (the reference trains with 128 per
 * bucket, run/ctc/cnn/train.py:72-73) runs as consecutive slabs of <= 32 rows through the default kernel pair where that pair serves
 * the shape (H % 128 == 0, offsets below 2 GiB) -- utterances are independent, the results are those of one launch, the time is
 * ceil(B / 32) recurrences -- and otherwise with one launch per time step,
 * 1 = one launch per time step, 2 = persistent with the placement-free hand-off only (sc1 write-through + agent-scope
 * counter; the wide kernels: 32 units x 4-row recurrences), 4 = persistent, XCD-local hand-off where the workgroups of a recurrence
 * find themselves on one XCD (decided inside the launch, falls back to the mode-2 protocol otherwise) signalled through a
 * line of per-producer flags, 8 = the same with the payload as its own signal (what mode 0 selects: consumers load until no
 * sentinel word is left: no flags, no store drain, one barrier per step), 7 = mode 4 with a forged split placement (test hook for
 * that fall-back).  Backward only: where H % 128 == 0 modes 0 / 8 run the partial-sum exchange kernel (a workgroup publishes the H
 * partial sums of dh of its 32 units, 4 KB per step in bf16, instead of every workgroup fetching the 3H gate gradients; dgh_bf16 is
 * then written by a storer wave and needs no sentinel fill); 9 = ask for that kernel, 10 = the same with a forged split placement
 * (its write-through stores).  Other values: ASR_ERR_BAD_ARG (3, 5 and 6 named kernel forms that no shape selected; removed).
 * Modes >= 2 return ASR_ERR_UNSUPPORTED instead of falling back to mode 1.
 * Widths: H % 32 == 0.  asr_gru_fwd (and asr_gru_fwd_state) serve H <= 1024; asr_gru_bwd (and asr_gru_bwd_state) stop at H <= 512
 * and return ASR_ERR_UNSUPPORTED above (the per-step backward kernel holds at most 12 K steps of 3H / 32 per wave, and no persistent
 * backward form is wider).  Persistent forms need a grid that fits the device's CUs (8 recurrences x H / 16 workgroups forward: H <= 512
 * on 256 CUs); the wide backward kernel needs H >= 64, the partial-sum one H in {128, 256, 384, 512}: modes 0 / 1 fall back to one launch
 * per time step where no persistent form serves (forward 512 < H <= 1024, backward H = 32), modes >= 2 refuse.  A refused call launches
 * no recurrence kernel; what it may have written by then is helper output only: with x_len the pinned update-gate columns of gi / the
 * masked copy of dy, and -- a refusal inside the forward launch helper -- cleared control words of sync_ws (never the abort word).
 * After a synchronisation ((int*)sync_ws)[1023] != 0 reports a timed-out in-launch wait (results invalid).  That word
 * is sticky: the calls zero every other control word but never this one, so a caller that reuses one sync_ws (zeroed
 * once) can look at it whenever convenient; once set, later launches give up immediately.
 */
size_t asr_gru_sync_bytes(int B, int H, int ndir);
/* gi: (T*B, ndir*3H) input projections, f32 (gi_bf16 = 0) or bf16 (gi_bf16 = 1: half the bytes written by the projection
 * GEMM and streamed here; accepted by the default persistent kernel only -- ask asr_gru_fwd_accepts_bf16_gi first, the call
 * returns -3 otherwise) */
int asr_gru_fwd_accepts_bf16_gi(int T, int B, int H, int ndir, int mode);
/* x_len (B) int32 or NULL: per-utterance frame counts -- chainer.links.NStepBiGRU (asr/nn/nn.py:3) runs every sequence over
 * its own length; with the padded (T, B) block of asr/data/processing.py:113-126 that means: row b is live for t < x_len[b], the
 * state is frozen beyond it (the reverse direction, which meets the padding first, therefore reaches t = x_len[b] - 1 with the zero
 * state it would start from), y is zero there and no gradient flows through those steps.  Implemented off the latency chain:
 * asr_gru_fwd overwrites the update-gate columns of gi on the dead rows (gi is scratch of the caller's projection GEMM: it is
 * MODIFIED when x_len is given) so that z == 1.0f exactly, asr_gru_bwd drops dy on the dead rows into dy_ws ((T*B, H) bf16,
 * required with x_len) -- every recurrence kernel form serves ragged batches unchanged. */
/* gates: (T*B, ndir, 4, H) = r | z | n | q saved for the backward pass, float32 -- or IEEE half (gates_f16 = 1: 2^-11 relative
 * rounding, half the bytes the forward storer writes and the backward loader reads beside the per-step hand-off) where the default
 * kernel pair serves the shape: ask asr_gru_gates_f16_ok (the calls return -3 otherwise); both calls must agree.  The half form is
 * BLOCKED by workgroup: (T*B, ndir, H/16, 4, 16) -- a row's r | z | n | q of 16 units are one 128-B line -- and private to the pair. */
int asr_gru_gates_f16_ok(int T, int B, int H, int ndir, int mode);
int asr_gru_fwd(void* stream, void* gi, int gi_bf16, const void* whh_bf16, const float* bhh, float* hseq, void* hseq_bf16,
                void* gates, void* y_bf16, int T, int B, int H, int ndir, void* sync_ws, int mode, const int* x_len, int gates_f16);
int asr_gru_bwd(void* stream, const void* dy_bf16, const void* gates, const float* hseq, const void* whhT_bf16,
                void* dgi_bf16, void* dgh_bf16, float* carry_ws, float* db_ih, float* db_hh, int T, int B, int H,
                int ndir, void* sync_ws, int mode, const int* x_len, void* dy_ws, int gates_f16);
/* The same layer with a GIVEN initial state (chainer.links.NStepGRU / NStepBiGRU: `hy, ys = rnn(hx, xs)`, exported by asr/nn/nn.py:3;
 * the reference's SRU model carries a state across calls, run/ctc/sru/model.py:105-122, no GRU recipe does).  hx (ndir, B, H) float32 or
 * NULL (= zeros); gi float32; gates float32 in the plain [T*B][ndir][4][H] layout.  They run on the one-launch-per-time-step kernels (the
 * persistent kernels start from a zero state).  The final state hy is rows of hseq: direction 0 at t = T - 1, direction 1 at t = 0 (with
 * x_len: the frozen state of a shorter utterance).  asr_gru_bwd_state: dhy (ndir, B, H) float32 or NULL = gradient arriving at hy; dhx
 * (ndir, B, H) float32 or NULL receives the gradient of hx; the caller adds dgh_{first step}^T . hx to the W_hh gradient (the
 * products over t >= 1 are those of asr_gru_bwd's caller). */
int asr_gru_fwd_state(void* stream, const float* gi, const void* whh_bf16, const float* bhh, const float* hx, float* hseq,
                      void* hseq_bf16, float* gates, void* y_bf16, int T, int B, int H, int ndir, const int* x_len);
int asr_gru_bwd_state(void* stream, const void* dy_bf16, const float* gates, const float* hseq, const float* hx, const float* dhy,
                      const void* whhT_bf16, void* dgi_bf16, void* dgh_bf16, float* carry_ws, float* db_ih, float* db_hh, float* dhx,
                      int T, int B, int H, int ndir, const int* x_len, void* dy_ws);

/* ---------------------------------------------------------------------------------------- SRU scan
 * Replaces the CUDA kernels `forward` / `backward` of asr/nn/sru.py:17-73,75-191 (SRUFunction.forward_gpu :327-367,
 * backward_gpu :372-433).  x, H, gH, gxh: (T, B, D) bf16;  U, gU: (T*B, 3D) [z | f | r] (U f32, gU bf16);
 * C (T, B, D) f32; bias (2D) [b_f | b_r]; c0, cT, gcT, gc0, mask: (B, D) f32 (c0 / mask / gH / gcT may be NULL).
 * asr_sru_combine: out = (a + b) * mask  (b NULL: out = a * mask) -- highway + projection gradient, input masking.
 * ws: asr_sru_ws_bytes(T, B, D) bytes of scratch (16-B aligned) for the chunked scans -- the cell recurrence is linear in c (and its
 * backward in gc), so time is cut into chunks that run in parallel, joined through per-chunk (product, sum) summaries (csrc/sru.hip);
 * NULL / too small / odd D / short T: the one-thread-per-column scans of the reference's shape serve.
 */
size_t asr_sru_ws_bytes(int T, int B, int D);
int asr_sru_fwd(void* stream, const void* x_bf16, const float* U, const float* bias, const float* c0, const float* mask,
                void* H_bf16, float* C, float* cT, int T, int B, int D, int use_tanh, void* ws, size_t ws_bytes);
int asr_sru_bwd(void* stream, const void* x_bf16, const float* U, const float* bias, const float* C, const float* c0,
                const float* mask, const void* gH_bf16, const float* gcT, void* gU_bf16, void* gxh_bf16, float* gbias,
                float* gc0, int T, int B, int D, int use_tanh, void* ws, size_t ws_bytes);
int asr_sru_combine(void* stream, const void* a_bf16, const void* b_bf16, const float* mask, void* out_bf16, long long n,
                    int BD);

/* ---------------------------------------------------------------------------------------- SRU as a sequence layer
 * The SRU above as a recurrent layer of the DS2 family (asr.functions.sru_seq, nn.SeqSRU / nn.BiSeqSRU; csrc/sru_seq.hip): per-utterance
 * lengths, ndir in {1, 2} directions, input width I != D, a carried cell state per direction.  The entries above are untouched.
 *
 * One layer has input width I, width D and ndir directions, each direction dir with parameters of its own, on (T, B, .) activations:
 *   U_t = W_dir x_t,  W_dir (k D, I) with rows [z; f; r] (k = 3) or [z; f; r; p] (k = 4).  k = 3 exactly when I == D (the reference's
 *   form, nn.SRU's parameter layout) and the highway input is xh_t = x_t; otherwise k = 4 and xh_t = U_p, the projection.
 *   f = sigmoid(U_f + b_f)   r = sigmoid(U_r + b_r)   c_t = f c_prev + (1 - f) z   h_t = r g(c_t) + (1 - r) xh_t,  g = tanh or identity.
 *   Direction 0 scans t = 0 .. x_len[b] - 1, direction 1 scans t = x_len[b] - 1 .. 0; both start from cx[dir, b] (NULL = zeros).
 *   x_len (B) int32 on the device, NULL = T for every utterance; an entry outside 0 .. T is CLAMPED to that range.
 *   Frames t >= x_len[b]: y is zero, the state is frozen, and the frame receives and passes no gradient (gU and gxh are zero there,
 *   gy is not read there) -- what functions.gru leaves in its padding.  C is not written there.
 *   cy[dir, b] = the state after the utterance's last own frame in scan order; x_len[b] = 0 gives cy = cx bit for bit (and dcx = dcy).
 *   y = sum over dir of h^dir.
 * Rounding points of y: every h^dir is formed in float32 registers from the float32 U, the float32 state and -- k = 3 -- the 16-bit x;
 * the sum over directions is taken in float32 in the same thread and y is rounded ONCE, to the 16-bit activation format, when it is
 * stored.  There is no 16-bit h per direction.  C and cy are float32 and never rounded.  Likewise backward: gxh = gy sum_dir (1 - r^dir)
 * is summed in float32 and rounded once; every block of gU is rounded once.
 * Operands: x (T, B, D) bf16, read only when k = 3 (may be NULL for k = 4); U (T*B, ndir k D) f32, direction-major column blocks
 * [dir][z | f | r (| p)] -- ONE product of the shared x with the stacked (ndir k D, I) weight; bias (ndir, 2D) [b_f | b_r];
 * cx, cy, dcy, dcx (ndir, B, D) f32 (cx, dcy, dcx may be NULL); C (ndir, T, B, D) f32 saved for the backward pass; y, gy (T, B, D) bf16;
 * gU (T*B, ndir k D) bf16, all k blocks (the p block: gy (1 - r)); gxh (T, B, D) bf16, the highway's gradient of x, written when k = 3
 * (may be NULL for k = 4); gbias (ndir, 2D) f32 is ACCUMULATED into.  The caller forms U and the weight / input gradients with
 * asr_gemm_nt / asr_gemm_tn_acc.
 * ws: asr_sru_seq_ws_bytes(T, B, D, ndir) bytes (0: none needed), required where that is not 0 (ASR_ERR_WORKSPACE).  Chunked scans as
 * above; odd D or operands off an 8-byte (float) / 4-byte (16-bit) boundary run one feature per lane instead of two, and T < 32 runs as
 * one chunk: the same kernels.  ASR_ERR_BAD_ARG: T, B or D <= 0, k not in {3, 4}, ndir not in {1, 2}, a NULL required pointer.
 * The IEEE-half build refuses (ASR_ERR_UNSUPPORTED).
 */
size_t asr_sru_seq_ws_bytes(int T, int B, int D, int ndir);
int asr_sru_seq_fwd(void* stream, const void* x_bf16, const float* U, const float* bias, const float* cx, const int* x_len,
                    void* y_bf16, float* C, float* cy, int T, int B, int D, int k, int ndir, int use_tanh, void* ws, size_t ws_bytes);
int asr_sru_seq_bwd(void* stream, const void* x_bf16, const float* U, const float* bias, const float* C, const float* cx,
                    const int* x_len, const void* gy_bf16, const float* dcy, void* gU_bf16, void* gxh_bf16, float* gbias, float* dcx,
                    int T, int B, int D, int k, int ndir, int use_tanh, void* ws, size_t ws_bytes);

/* ---------------------------------------------------------------------------------------- optimiser step
 * GradientClipping -> WeightDecay -> Adam over one flat buffer (run/ctc/cnn/train.py:142-147,200).
 * grad_scale multiplies every gradient first (1/world_size after a sum all-reduce).
 */
int asr_fill_f32(void* stream, float* p, long long n, float value);
int asr_sqnorm_acc(void* stream, const float* g, long long n, float* out);
int asr_clip_decay_adam(void* stream, float* p, const float* g, float* m, float* v, long long n, float alpha,
                        float beta1, float beta2, float eps, float weight_decay, float clip_threshold,
                        float grad_scale, const float* sqnorm, int step);
/* kind 0 SGD, 1 MomentumSGD, 2 NesterovAG (asr/optimizers.py:43-52), same clipping / decay front end */
int asr_clip_decay_sgd(void* stream, float* p, const float* g, float* v, long long n, int kind, float lr, float momentum,
                       float weight_decay, float clip_threshold, float grad_scale, const float* sqnorm);
/* The same step with its decisions taken on the device by one thread (no host synchronisation, no host-side step count):
 * asr_step_control takes the squared norm of the flat gradient g (n floats; per-workgroup partial sums into `partials`,
 * asr_sqnorm_partials_count(n) floats, then summed in a fixed order -- bit-identical on every data-parallel rank, which
 * float atomics are not), reads up to two abort words of persistent GRU launches (sync_ws int 1023 of asr_gru_fwd /
 * asr_gru_bwd; NULL = none) and writes ctl[8] = {drop, gradient factor, Adam's alpha_t, t, squared norm, ...}: the step is
 * dropped when the norm is not finite (the reference's NaN check, run/ctc/cnn/train.py:193-197) or an abort word is raised
 * (the recurrence's outputs are garbage); *applied_steps (device int, zero at start) counts the steps that were NOT dropped
 * and is the t of Adam's bias correction (the reference `continue`s before optimizer.update).  asr_adam_ctl / asr_sgd_ctl
 * apply the step ctl describes.  ctl[5] = 1 when the drop was caused by a recurrence that gave up -- here (abort words) or on
 * another data-parallel rank: reserved_index >= 0 names an element of g that belongs to no parameter; asr_gather_abort ORs any
 * number of abort words (device array of n device addresses) into *any_word and, when one is raised, plants a NaN in *poison
 * (that element of the LOCAL gradient buffer, before it is summed over the ranks), so every rank drops the same step and every
 * rank can tell why; ctl[6] (zeroed once by the caller) counts such steps, so a host that reads ctl late misses none. */
int asr_sqnorm_partials_count(long long n);
int asr_gather_abort(void* stream, const long long* word_ptrs, int n, int* any_word, float* poison);
int asr_step_control(void* stream, const float* g, long long n, float* partials, const int* abort0, const int* abort1,
                     float clip_threshold, float grad_scale, float alpha, float beta1, float beta2, int* applied_steps,
                     float* ctl, int reserved_index);
/* asr_step_control with loss scaling (chainer.Optimizer.loss_scaling(interval, scale); the IEEE-half build of BASELINE configs[4]):
 * loss_scale = device float[4] {scale S, applied steps since S last changed, growth interval (0 = S is static), overflows so far}.
 * The caller seeds the backward pass with S (the gradient handed to asr_ctc_backward's gy is the device float loss_scale[0] itself,
 * read when that kernel runs); this call divides the gradient factor by S, and when the norm is not finite without a recurrence
 * having given up -- an activation gradient overflowed the half range -- drops the step and halves S (down to 2^-24: a model whose
 * unscaled activation gradients leave the half range needs S < 1); `interval` applied steps in a row double it (up to 2^24).  No host synchronisation; identical on every data-parallel rank.
 * loss_scale == NULL: asr_step_control. */
int asr_step_control_scaled(void* stream, const float* g, long long n, float* partials, const int* abort0, const int* abort1,
                            float clip_threshold, float grad_scale, float alpha, float beta1, float beta2, int* applied_steps,
                            float* ctl, int reserved_index, float* loss_scale);
int asr_adam_ctl(void* stream, float* p, const float* g, float* m, float* v, long long n, float beta1, float beta2, float eps,
                 float weight_decay, const float* ctl);
int asr_sgd_ctl(void* stream, float* p, const float* g, float* v, long long n, int kind, float lr, float momentum,
                float weight_decay, const float* ctl);

/* ---------------------------------------------------------------------------------------- the rest of asr.nn's function layers
 * asr/nn/nn.py:18-23 CReLU, :42-43 LogSoftmax, :58-63 Softmax (axis 1 = the channels = the contiguous axis of the physical layout),
 * :77-93 AveragePooling2D / ND (ksize (k, 1), stride = ksize, pad 0; Chainer's average pooling has no cover_all: Hout = (Hin - k) / k
 * + 1), :123-133 Unpooling2D (ksize (k, 1), stride = ksize; Hout = k (Hin - 1) + 1 with cover_all, k Hin without), :220-231
 * GaussianNoise (x + N(0, std^2), counter-based).  No recipe of the reference uses them; rows = every axis but the channels;
 * x, y, dy, dx bf16. */
int asr_crelu_fwd(void* stream, const void* x, void* y, long long rows, int C);
int asr_crelu_bwd(void* stream, const void* x, const void* dy, void* dx, long long rows, int C);
int asr_softmax_fwd(void* stream, const void* x, void* y, long long rows, int C, int log_form);
int asr_softmax_bwd(void* stream, const void* y, const void* dy, void* dx, long long rows, int C, int log_form);
int asr_avgpool_h_fwd(void* stream, const void* x, void* y, long long R, int Hin, int C, int k);
int asr_avgpool_h_bwd(void* stream, const void* dy, void* dx, long long R, int Hin, int C, int k);
int asr_unpool_h_fwd(void* stream, const void* x, void* y, long long R, int Hin, int Hout, int C, int k);
int asr_unpool_h_bwd(void* stream, const void* dy, void* dx, long long R, int Hin, int Hout, int C, int k);
int asr_gaussian_noise(void* stream, const void* x, void* y, long long n, float stdv, unsigned int seed);
/* asr/nn/nn.py:135-146 UpSampling2D = chainer.functions.upsampling_2d: the inverse of a max pooling given its argmax positions
 * (`indexes` of a MaxPooling2D function object; ksize (k, 1), stride = ksize: the row inside the window).  asr_maxpool_h_indexes forms
 * them as uint8 (R, Hout, C) with Hout = the cover_all output height; upsample forward: y (R, Hout', C) with x[r][h][c] at row
 * h k + idx and zeros elsewhere; backward: dx[r][h][c] = dy[r][h k + idx][c]. */
int asr_maxpool_h_indexes(void* stream, const void* x, void* idx_u8, long long R, int Hin, int C, int k);
int asr_upsample_h_fwd(void* stream, const void* x, const void* idx_u8, void* y, long long R, int Hin, int Hout, int C, int k);
int asr_upsample_h_bwd(void* stream, const void* dy, const void* idx_u8, void* dx, long long R, int Hin, int Hout, int C, int k);
/* asr/nn/nn.py:115-121 SpatialPyramidPooling2D = chainer.functions.spatial_pyramid_pooling_2d with max pooling: level l < pyramid_height
 * pools the (H, T) plane of every (utterance, channel) over 2^l x 2^l bins (window ceil(size / 2^l), stride = window, -inf padding of
 * (2^l k - size + 1) / 2).  x: the physical (T, B, H, C) bf16 tensor; y: (B, asr_spp_bins(pyramid_height), C) bf16, bins level after
 * level, [by][bx] inside a level; pos (same shape, int32, may be NULL): flat h T + t position of each maximum (first one in (h, t)
 * order) for asr_spp_bwd, which ADDS dy into dx32 (T, B, H, C) float32 (zeroed by the caller: levels overlap). */
int asr_spp_bins(int pyramid_height);
int asr_spp_fwd(void* stream, const void* x, void* y, int* pos, int T, int B, int H, int C, int pyramid_height);
int asr_spp_bwd(void* stream, const void* dy, const int* pos, float* dx32, int T, int B, int H, int C, int pyramid_height);

/* ---------------------------------------------------------------------------------------- lookahead (row) convolution
 * Deep Speech 2's lookahead layer on (T, B, D) 16-bit activations; w (D, tau + 1) float32, no bias; x_len (B) int32 or NULL (= T):
 *   y[t, b, d]  = sum_{j=0..tau} w[d, j] * x[t + j, b, d]     with x = 0 at t + j >= x_len[b];  y = 0 at t >= x_len[b]
 *   dx[t, b, d] = sum_{j=0..tau} w[d, j] * gy[t - j, b, d]    gy at and beyond x_len[b] is ignored; dx = 0 at t >= x_len[b]
 *   dW[d, j]   += sum_{t, b} gy[t, b, d] * x[t + j, b, d]     over t + j < x_len[b]
 * float32 accumulation in a fixed tap order (forward j = 0..tau), one rounding at the store: an output element does not depend on T,
 * on the time tile (ASR_LOOKAHEAD_TIME_TILE rows) it fell into or on where a longer sequence was cut.  dW is summed in two stages
 * (per-workgroup partial sums in `ws`, asr_lookahead_ws_bytes; then one ordered sum added once to dW): no float atomics, the same
 * bits on every run.  asr_lookahead_bwd: dx_bf16 NULL = no input gradient, dW NULL = no weight gradient (then x_bf16 and ws may be
 * NULL).  Limits: D % 8 == 0 and tau <= ASR_LOOKAHEAD_MAX_TAU, else ASR_ERR_UNSUPPORTED (nothing is written; _ws_bytes returns 0). */
#define ASR_LOOKAHEAD_MAX_TAU 96
#define ASR_LOOKAHEAD_TIME_TILE 64
size_t asr_lookahead_ws_bytes(int T, int B, int D, int tau);
int asr_lookahead_fwd(void* stream, const void* x_bf16, const float* w, const int* x_len, void* y_bf16, int T, int B, int D, int tau);
int asr_lookahead_bwd(void* stream, const void* gy_bf16, const void* x_bf16, const float* w, const int* x_len, void* dx_bf16,
                      float* dW, void* ws, size_t ws_bytes, int T, int B, int D, int tau);

/* ---------------------------------------------------------------------------------------- carried rows of a streaming forward
 * A delay line of K rows of R 16-bit features per batch slot: state (K, B, R), of which the first m[b] <= K rows are valid.
 * asr_stream_push takes a chunk (Tc, B, R) of which n[b] rows are valid (n NULL = all Tc) and writes, per slot b,
 *   window (K + Tc, B, R): [m[b] carried rows | n[b] new rows | zeros], left-aligned;  wlen[b] = m[b] + n[b];
 *   emit[b]: the rows the layer behind the window may emit;  the new state: the last min(K, wlen[b]) valid rows, and m[b].
 * mode ASR_STREAM_CONTEXT (the left context of a causal convolution): m == K always (the argument m is not read; a reset slot
 * holds K zero rows that count as valid) and emit[b] = n[b].  mode ASR_STREAM_LOOKAHEAD (the pending frames of a lookahead layer):
 * emit[b] = max(0, m[b] + n[b] - K).  A slot with n[b] == 0 keeps its state bytes.  flush (B) int32 or NULL, lookahead mode only --
 * the end of utterances: no slot is fed (chunk may be NULL, Tc 0), emit[b] = m[b] where flush[b] != 0 (0 elsewhere) and those
 * slots are then emptied.  asr_stream_push_reset zeroes the rows of every slot, or of those with mask[b] != 0, and sets m[b] = 0
 * (m NULL: context mode).  Bit-exact copies.  R % 8 == 0, else ASR_ERR_UNSUPPORTED. */
#define ASR_STREAM_CONTEXT 0
#define ASR_STREAM_LOOKAHEAD 1
int asr_stream_push(void* stream, void* state, int* m, const void* chunk, const int* n, const int* flush, void* window, int* wlen,
                    int* emit, int K, int Tc, int B, int R, int mode);
int asr_stream_push_reset(void* stream, void* state, int* m, const int* mask, int K, int B, int R);

/* ---------------------------------------------------------------------------------------- time reduction by frame stacking
 * k consecutive frames of R 16-bit features become one frame of k * R features.  x (T, B, R), y (G, B, k * R), G = ceil(T / k);
 * x_len (B) int32 or NULL (= T), clamped to [0, T]:
 *   asr_time_stack_fwd   y[g, b, j * R + r] = x[g * k + j, b, r] where g * k + j < x_len[b], 0 elsewhere: a partly filled last group
 *                        is completed with zeros (the zero future of the lookahead layer), whole groups at or beyond
 *                        ceil(x_len[b] / k) are zero.  y_len (B) int32, if not NULL, receives ceil(x_len[b] / k).  T == 0 writes
 *                        only y_len.
 *   asr_time_stack_bwd   the inverse copy: dx[t, b, r] = gy[t / k, b, (t % k) * R + r] for t < x_len[b], 0 for x_len[b] <= t < T.
 *                        Every element of dx is written; no atomics.
 * asr_time_stack_push is the streaming form.  Per slot b, state (k - 1, B, R) holds m[b] < k pending rows.  The call takes n[b]
 * rows of chunk (Tc, B, R) (n NULL = Tc; clamped to [0, Tc]) and writes y (ceil((k - 1 + Tc) / k), B, k * R): the forward above of
 * the sequence [m[b] pending | n[b] new], left-aligned -- so the trailing partial group IS written, zero-completed, behind the
 * emit[b] = (m[b] + n[b]) / k whole groups, and whole zero groups behind it; the consumer runs with length emit[b].  The last
 * (m[b] + n[b]) % k rows become the new state (the rows behind them are zeroed) and the new m[b].  A slot with n[b] == 0 keeps its
 * state bytes.  flush (B) int32 not NULL = end of utterances: no slot is fed (chunk may be NULL, Tc 0); where flush[b] != 0 and
 * m[b] > 0 the pending rows are emitted as one zero-completed group (emit[b] = 1) and the slot is emptied (state rows zeroed,
 * m[b] = 0); elsewhere emit[b] = 0, y is zero and the state stays.  Two launches: the first reads the state and writes y and emit,
 * the second reads y and writes the state and m (one workgroup per slot), so a short chunk never reads what it has overwritten.
 * asr_time_stack_push_reset zeroes the pending rows and m[b] (m may be NULL) of every slot, or of those with mask[b] != 0.
 * k == 1: fwd and bwd are plain copies, the push state is empty (state and m may be NULL, emit[b] = n[b]).
 * Bit-exact copies, independent of the activation type.  R % 8 != 0 or k outside [1, ASR_TIME_STACK_MAX]: ASR_ERR_UNSUPPORTED;
 * a NULL tensor that would be accessed, a negative T or Tc, B < 1 or R < 1: ASR_ERR_BAD_ARG; nothing is written in either case. */
#define ASR_TIME_STACK_MAX 8
int asr_time_stack_fwd(void* stream, const void* x, const int* x_len, void* y, int* y_len, int T, int B, int R, int k);
int asr_time_stack_bwd(void* stream, const void* gy, const int* x_len, void* dx, int T, int B, int R, int k);
int asr_time_stack_push(void* stream, void* state, int* m, const void* chunk, const int* n, const int* flush, void* y, int* emit,
                        int Tc, int B, int R, int k);
int asr_time_stack_push_reset(void* stream, void* state, int* m, const int* mask, int B, int R, int k);

/* ---------------------------------------------------------------------------------------- latency-controlled bidirectional GRU
 * The layer (asr.nn.LCBiGRU, asr.functions.lc_bigru) on x logical (B, D, T), len[b] = x_length[b] clamped to 0..T (T without
 * lengths), a block of Nc >= 1 frames, Nr >= 0 frames of right context, W = min(Nc + Nr, T):
 *   forward direction   as nn.GRU with the direction-0 parameters over t = 0 .. len[b] - 1 from a zero state.
 *   reverse direction   for every block c = 0 .. ceil(len[b] / Nc) - 1, with e = min((c + 1) Nc + Nr, len[b]): the state is zero at e,
 *                       the direction-1 recurrence runs t = e - 1 down to c Nc, and its outputs are kept for
 *                       c Nc <= t < min((c + 1) Nc, len[b]); the Nr right-context steps only warm the state up.
 *   output              y[t] = h_fwd[t] + h_rev[t] (summed, as BiGRU does), zero at t >= len[b]; no gradient enters or leaves the
 *                       padding.  With Nc >= T the layer is mathematically nn.BiGRU.
 * The reverse direction runs as a batch of C * B windows, C = ceil(T / Nc), window (c, b) at index c * B + b, each time-reversed so
 * that the ndir = 1 recurrence serves it with per-window lengths.  Window (c, b) has L = clamp(len[b] - c Nc, 0, W) live rows; with
 * n_win (B) int32 not NULL, L = 0 for c >= n_win[b].  x, y, addend (T, B, R) and xw, yw (W, C * B, R) are 16-bit activations.
 *   asr_lc_gather   xw[j, c B + b] = x[c Nc + L - 1 - j, b] for j < L and L - 1 - j < keep, zero elsewhere; w_len[c B + b] = L
 *                   (w_len may be NULL).  mode ASR_LC_WINDOW: keep = W (the inputs).  mode ASR_LC_BLOCK: keep = Nc (the output
 *                   gradient: the adjoint of the crop, right-context outputs receive none).
 *   asr_lc_scatter  for t < len[b]: y[t, b] = addend[t, b] (0 if addend is NULL) + the sum over c, ascending, of
 *                   yw[L_c - 1 - (t - c Nc), c B + b] over the windows with c Nc <= t < c Nc + L_c.  mode ASR_LC_BLOCK: only the
 *                   frame's own block c = t / Nc (the forward pass: the two directions summed).  mode ASR_LC_WINDOW: every such
 *                   window (the overlap-add of the input gradient, up to 1 + ceil(Nr / Nc) terms).  float32 accumulation in that
 *                   order, one rounding to the activation type.  y is zero at t >= len[b]; every element of y is written.
 * The two are adjoint in pairs: gather(ASR_LC_BLOCK) of scatter(ASR_LC_BLOCK), gather(ASR_LC_WINDOW) of scatter(ASR_LC_WINDOW).
 * asr_lc_push is the streaming carry.  Per slot b, state (K, B, R), K = Nc + Nr - 1, holds m[b] <= K pending rows.  The call takes
 * n[b] rows of chunk (Tc, B, R) (n NULL = Tc; clamped to [0, Tc]) and writes window (K + Tc, B, R) = [m[b] pending | n[b] new | zeros],
 * a[b] = m[b] + n[b], w[b] = max(0, a[b] - Nr) / Nc (the whole blocks whose right context is present) and emit[b] = w[b] Nc; for a
 * slot with flush[b] != 0 (flush (B) int32 or NULL), whose [pending | new] rows are its utterance's end: w[b] = ceil(a[b] / Nc) and
 * emit[b] = a[b].  Rows emit[b] .. a[b] - 1 become the new state (the rows behind them are zeroed) and their count the new m[b].  A
 * slot with n[b] == 0 and no flush keeps its state bytes.  Two launches: the first reads the state and writes the window, a, w and
 * emit; the second reads those and writes the state and m.  Reset: asr_stream_push_reset(state, m, mask, K, B, R).
 * ASR_ERR_BAD_ARG, and nothing launched or written: Nc < 1, Nr < 0, R < 8 or R % 8 != 0, B < 1, a negative T or Tc, T above 2^30,
 * a mode other than the two, W (or, for the push, Nc + Nr) above ASR_LC_MAX_WINDOW, C * B or a tensor's count of 16-byte lanes that
 * does not fit 31 bits, a NULL tensor that would be accessed.  T == 0 (gather, scatter) is ASR_OK and writes nothing. */
#define ASR_LC_MAX_WINDOW 4096
#define ASR_LC_WINDOW 0
#define ASR_LC_BLOCK 1
int asr_lc_gather(void* stream, const void* x, const int* x_len, const int* n_win, void* xw, int* w_len, int T, int B, int R, int Nc,
                  int Nr, int mode);
int asr_lc_scatter(void* stream, const void* yw, const void* addend, const int* x_len, const int* n_win, void* y, int T, int B, int R,
                   int Nc, int Nr, int mode);
int asr_lc_push(void* stream, void* state, int* m, const void* chunk, const int* n, const int* flush, void* window, int* a, int* w,
                int* emit, int Tc, int B, int R, int Nc, int Nr);

/* ---------------------------------------------------------------------------------------- streaming log-mel front end
 * Samples in chunk by chunk, feature frames out, for B batch slots that start and end on their own: for every way of cutting a
 * signal the emitted frames are, bit for bit, those of asr_specgram_bands + asr_deltas on the whole signal (L = frame_len,
 * S = frame_step <= L, c = preemph).  Log-mel frame f depends on samples [f S - 1, f S + L); feature frame t (static, delta,
 * delta-delta) on log-mel frames t - 2 .. t + 2, clamped at 0 on the left; the right-edge clamp of the one-shot deltas never reaches
 * an emitted frame (the last two frames are dropped).  Feature frame t is therefore out once sample (t + 2) S + L - 1 is in.
 * State per slot b (the caller owns the buffers; reset or zero-filled state is an empty slot):
 *   pend (B, pend_pitch >= L) float32   the pre-emphasised samples of frames not yet complete, meta[b][0] = m[b] < L of them
 *   last (B) float32                    the last raw sample: the predecessor of the next chunk's first sample (valid: meta[b][1])
 *   logmel (B, Fmax, nfilt) float32     rows [4 - r[b], 4) of a slot: its last r[b] = min(4, meta[b][2]) log-mel rows
 *   meta (B, ASR_FBANK_STREAM_META) int32: {m, a predecessor exists, log-mel frames so far, feature frames emitted since the reset,
 *                                       ended: flushed and not fed since, 0, 0, 0}
 * asr_fbank_stream_push, chunk (B rows of chunk_pitch >= Nc samples, int16 or float32), n (B) int32 or NULL (= Nc), clamped to [0, Nc]:
 *   1. y[i] = x[i] - c x[i - 1] with the instructions of the one-shot kernels; the predecessor of the chunk's first sample is `last`;
 *      y = x for the first sample after a reset.
 *   2. window row b = [m pending | n new | zeros up to four past a multiple of 4], wlen[b] = m + n; the complete frames in it:
 *      k[b] = 0 if wlen < L, else 1 + (wlen - L) / S; the new pending part is window[k S : wlen], always shorter than L.
 *   3. (the caller) asr_specgram_bands(window, sig_is_f32 = 1, lengths = wlen, sig_pitch = win_pitch, preemph = 0.0, nframes = k,
 *      Fmax, logmel_out = logmel + 4 * nfilt): with a zero coefficient the samples pass unchanged, so every frame goes through the
 *      one-shot transform, mel and logarithm code on the same float32 inputs; the k new rows land behind the slot's 4 carried rows.
 *      win_pitch % 4 == 0 and a 16-byte aligned window keep the nfft = 512 kernel selected whenever the one-shot call selects it.
 *   A slot with n[b] == 0 keeps every byte of its state (wlen[b] = m, k[b] = 0).
 *   flush (B) int32, non-NULL = end of utterance for the slots with flush[b] != 0 (chunk NULL, Nc 0): wlen[b] = m and k[b] = 1 iff the
 *   slot has no log-mel frame yet or m > L - S -- the one zero-padded frame framesig adds: F - (complete frames), F = 1 + ceil((N - L) / S)
 *   or 1 for N <= L -- and the slot's samples are dropped; other slots: k[b] = 0, state kept.
 * asr_fbank_stream_deltas, after step 3, with c the log-mel frames before the call and c' = c + k[b]:
 *   4. out (B, 3, nfilt, Tc) float32, left-aligned: columns 0 .. lengths[b] - 1 are feature frames max(0, c - 2) .. max(0, c' - 2) - 1
 *      from [carried rows | new rows]: at(q) = lm[max(q, 0)], dl(q) = (at(max(q, 0) + 1) - at(max(q, 0) - 1)) * 0.5,
 *      v0 = at(t), v1 = dl(t), v2 = (dl(t + 1) - dl(t - 1)) * 0.5, then (v - mean) / std if mean and stdv (3 * nfilt each) are given;
 *      columns at or beyond lengths[b] hold the one-shot's padding: 0, or (0 - mean) / std.  The last min(4, c') rows are carried and
 *      the counters advance.  With flush non-NULL the flushed slots emit their last 0 or 1 frame -- max(F - 2, 0) in all, the one-shot's
 *      x_length -- and start over; their feature-frame count stands (ended = 1) until asr_fbank_stream_push feeds the slot again.
 * asr_fbank_stream_reset empties every slot, or those with mask[b] != 0.
 * Limits, checked before any launch: nfilt <= ASR_FBANK_STREAM_MAX_FILT; at most ASR_FBANK_STREAM_MAX_FRAMES new frames per call
 * (1 + (Nc - 1) / S and Tc; (4 + 128) rows of 65 floats = 34 KB of LDS); S <= L <= 1024 as in asr_specgram: else ASR_ERR_UNSUPPORTED.
 * pend_pitch < L, win_pitch < (L - 1 + Nc rounded up to 4) + 4, win_pitch % 4 != 0 or a window off 16 bytes: ASR_ERR_WORKSPACE.  NULL
 * or non-positive arguments: ASR_ERR_BAD_ARG.  One workgroup per slot: no launch reads what another workgroup of it writes.  Nothing is
 * allocated, copied to the host or synchronised. */
#define ASR_FBANK_STREAM_MAX_FRAMES 128
#define ASR_FBANK_STREAM_MAX_FILT 64
#define ASR_FBANK_STREAM_META 8
int asr_fbank_stream_push(void* stream, const void* chunk, int chunk_is_f32, long long chunk_pitch, int Nc, const int32_t* n,
                          const int32_t* flush, float* pend, int pend_pitch, float* last, int32_t* meta, float* window,
                          long long win_pitch, int32_t* wlen, int32_t* k, int B, int frame_len, int frame_step, double preemph);
int asr_fbank_stream_deltas(void* stream, float* logmel, const int32_t* k, const int32_t* flush, int32_t* meta, int B, int Fmax,
                            int nfilt, int Tc, const float* mean, const float* stdv, float* out, int32_t* lengths);
int asr_fbank_stream_reset(void* stream, int32_t* meta, const int32_t* mask, int B);

#ifdef __cplusplus
}
#endif
#endif
