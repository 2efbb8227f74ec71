/*
 * sot_hip.h -- C ABI of libsot_hip.so, the MI355X (gfx950) implementation of the
 * 1-D spectral optimal-transport loss.
 *
 * This is the drop-in boundary for the reference's hot path.  The reference is pure
 * Python on PyTorch (no FFI of its own), so each entry point replaces a *composition of
 * ATen ops* in the reference; the Python binding a maintainer adds is shown in
 * INTEGRATION.md (ctypes; the shipped host-side mirror is
 * 1d-spectral-optimal-transport_amd/losses.py).
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless stated;
 *   - the caller owns and allocates everything (outputs and workspace); functions only
 *     enqueue work on `stream` (a hipStream_t passed as void*; NULL = default stream):
 *     no allocation, no host synchronisation, graph-capturable;
 *   - return value: SOT_OK (0) or a negative sot_status; nothing aborts, nothing is
 *     enqueued when an error is returned;
 *   - rows are independent: a caller shards a batch by passing a sub-range of rows;
 *   - memory: a call writes only the elements of its outputs and the first *_workspace_bytes() bytes of its workspace; it reads
 *     nothing outside its rows whose value can reach a result (the gaps between strided rows and whatever surrounds a buffer may
 *     hold anything, NaN included); it leaves its inputs unchanged.  Alignment: every buffer needs the alignment of its element
 *     type and no more unless stated with the buffer; a better-aligned call may take a faster kernel, a worse-aligned one is still
 *     correct.  tests/test_memory_contract_gpu.py holds every entry point to this with guard bands around each buffer.
 */
#ifndef SOT_HIP_H
#define SOT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SOT_ABI_VERSION 21  /* bumped on every change of a signature or of a buffer contract below; the binding checks it
                              * (11, round 6: sot_workspace_bytes covers the per-row pre-sort; the MSS workspace is 16-byte aligned;
                              *  14: sot_w1d_quantiles_backward; 15: sot_fir_*; 16: sot_spec_metrics; 17: sot_w1d_mixed_*;
                              *  18: sot_workspace_bytes is 0 for per-row positions outside the pre-sort's domain;
                              *  19: bfloat16 weight rows -- sot_rows_bf16_to_f32, sot_rows_f32_to_bf16, sot_w1d_*_bf16;
                              *  20: bfloat16 training -- sot_w1d_backward_bf16, sot_w1d_loss_and_grad_bf16, sot_w1d_bf16_native,
                              *      sot_w1d_bf16_backward_workspace_bytes;
                              *  21: float64 rows -- sot_problem_f64, sot_w1d_forward_f64, sot_w1d_backward_f64, sot_w1d_f64_supported,
                              *      sot_w1d_f64_workspace_bytes) */

typedef enum sot_status {
    SOT_OK = 0,
    SOT_ERR_INVALID_P = -1,        /* p < 1          -> AssertionError in the reference (losses.py:271) */
    SOT_ERR_BAD_SHAPE = -2,        /* B < 0, n < 1, m < 1, bad strides                                 */
    SOT_ERR_UNSUPPORTED_SIZE = -3, /* a row's working set exceeds one CU's 160 KiB LDS (n + m > ~19000) */
    SOT_ERR_NULL_POINTER = -4,
    SOT_ERR_WORKSPACE = -5,        /* workspace smaller than sot_workspace_bytes()                     */
    SOT_ERR_LAUNCH = -6            /* hipGetLastError() != hipSuccess after the launch                 */
} sot_status;

/* flag bits: the keyword arguments of Wasserstein1D (losses.py:90-121, 129-196) */
#define SOT_FLAG_SQUARE 1u         /* square_dist: weights are squared first       (losses.py:172-174) */
#define SOT_FLAG_DONT_NORMALIZE 2u /* y is divided by the mass of x, not its own   (losses.py:180-184) */
#define SOT_FLAG_LIMIT_Q 4u        /* levels Q_k > 1 contribute nothing            (losses.py:306-307) */
#define SOT_FLAG_REQUIRE_SORT 8u   /* sort supports, permute weights               (losses.py:286-290) */
#define SOT_FLAG_PRENORMALIZED 16u /* weights are used as given: the functional wasserstein_1d(u_values,
                                      v_values, u_weights, v_weights) of losses.py:223, which does not
                                      normalise (flags SQUARE / DONT_NORMALIZE are then ignored)       */
#define SOT_FLAG_NO_SPECIALIZE 32u /* diagnostic: always run the generic kernels, never the variants with the row
                                      length at compile time (257/512/513/1025/2048/8192 bins).  Results are
                                      bit-identical for 512/2048/8192 and agree to the last bits otherwise;
                                      the tests compare the two                                              */

#define SOT_FLAG_SAME_GRID 64u     /* the caller guarantees that xpos and ypos hold the SAME values (n == m, equal element by
                                      element after sorting; shared positions only): what every reference call site passes
                                      (y_pos = x_pos.clone(), trainer.py:191; the fixed_x buffer).  For p == 1 without
                                      SOT_FLAG_LIMIT_Q the forward then evaluates the area between the two CDFs on that grid,
                                      sum_i |U_i - V_i| (pos_{i+1} - pos_i) -- the same W_1, no merge (<= 3e-7 from the merge
                                      kernel's value).  A wrong guarantee gives wrong results                                */
#define SOT_FLAG_NO_AREA 128u      /* diagnostic: ignore SOT_FLAG_SAME_GRID (always the merge kernel)                         */
#define SOT_FLAG_TIE_FREE_GRADIENT 256u /* OPT-IN: the caller accepts, at exactly tied float32 CDF levels, the derivative of the loss
                                      as a function of the CDF values (what float64 autograd of the reference returns) instead of the
                                      tie-order artefact of the reference's float32 autograd (losses.py:295-298: ranks are constants
                                      to autograd, so a run of equal levels hands its whole gradient to one member).  With it, p == 1
                                      with SOT_FLAG_SAME_GRID and no cutoff gets a MERGE-FREE training form (gradient w.r.t. y alone):
                                      8192 x 2048 rows 72.7 -> 47.5 us, 16384 x 1025 rows 76 -> 69 us.  Gradient entries of rows without tied
                                      levels are unchanged; the loss value is the merge-free forward kernel's (<= 3e-7 from the merge walk's).
                                      The flag is a PERMISSION: the merge-free form serves the row lengths with a compile-time training kernel, and for
                                      the power-of-two lengths (512 ... 4096) only when the rows of x, y and grad_y start on 16-byte boundaries (row
                                      strides multiples of 4); any other call -- another length, rows 4 bytes off -- returns the reference's tie order
                                      on tied rows, as without the flag.  129, 257, 513, 1025 and 2049 bins are served at every alignment */

/* One batch of spectrum pairs.  Mirrors the arguments of Wasserstein1D.forward
 * (losses.py:129) after its [batch,time,N] -> [B,N] reshape (losses.py:157-170). */
typedef struct sot_problem {
    const float *x;           /* [B, n] weights of the first measure (magnitude spectrum)             */
    const float *y;           /* [B, m] weights of the second measure                                 */
    const float *xpos;        /* support positions of x: [n] (row stride 0) or [B, n]                 */
    const float *ypos;        /* support positions of y: [m] (row stride 0) or [B, m]                 */
    int64_t B;                /* rows (spectrum pairs) in this call                                   */
    int32_t n, m;             /* support sizes (row lengths)                                          */
    int64_t x_row_stride;     /* elements between consecutive rows of x (>= n)                        */
    int64_t y_row_stride;     /* elements between consecutive rows of y (>= m)                        */
    int64_t xpos_row_stride;  /* 0 = one position row shared by all rows (the stride-0 expand of      */
    int64_t ypos_row_stride;  /*     losses.py:167-170), otherwise >= n / >= m                        */
    float p;                  /* order of the distance, p >= 1; result is W_p^p (no root)             */
    uint32_t flags;           /* SOT_FLAG_*                                                           */
    /* Optional position plan from sot_prepare_positions() (shared positions only).  When
     * perm_is_identity != NULL, xpos/ypos must be the SORTED positions that call produced and
     * SOT_FLAG_REQUIRE_SORT costs nothing extra (no internal sort, no workspace). NULL otherwise. */
    const int32_t *xperm;            /* [n] sort permutation of the original xpos             */
    const int32_t *yperm;            /* [m]                                                    */
    const int32_t *perm_is_identity; /* [2] device flags: 1 = positions were already sorted    */
    /* Round 5, per-row positions with SOT_FLAG_REQUIRE_SORT (the `torch.sort(u_values, 1)` of losses.py:286-288 on every row): the sort runs
     * ONCE per training step.  row_perm_out (or NULL): a call that sorts stores each row's two sort permutations here, [B, n + m] uint16 (the n
     * original columns of x's sorted supports, then the m of y's; n, m <= 16384).  row_perm_in (or NULL): permutations an earlier call produced
     * for the SAME position tensors -- sot_w1d_backward / sot_w1d_position_grad (and the forward itself) then gather the sorted supports
     * through them instead of sorting again.  Ignored for shared positions.
     * Round 6: rows of 2 ... 2048 positions are sorted AHEAD of the row kernel by a kernel of their own (one wavefront per row, a packed-word
     * network in registers: csrc/sot_wave_sort.hpp) whenever there is a place for the permutations -- row_perm_out, else the call's workspace
     * when it holds sot_workspace_bytes() bytes, else the row kernel sorts in LDS as before.  Either way an image that a call has written holds
     * the stable sort permutations of every row.
     * Alignment of the image (row_perm_out, row_perm_in, or the workspace standing in for it): 2 bytes are enough.  On a 16-byte boundary, with
     * n == m in {512, 1024, 2048} and 16-byte aligned weight rows, the calls take the compile-time-length kernels; on an 8-byte boundary with
     * n, m multiples of 4 and 16-byte aligned position rows the pre-sort stores packed words; anything less runs the element-wise forms. */
    uint16_t *row_perm_out;
    const uint16_t *row_perm_in;
} sot_problem;

int sot_abi_version(void);
const char *sot_status_string(int status);

/* Bytes of device workspace the calls below need for this problem (host-side arithmetic only).  Shared positions with
 * SOT_FLAG_REQUIRE_SORT and no plan: required.  Per-row positions with SOT_FLAG_REQUIRE_SORT and neither row_perm_in nor row_perm_out
 * (round 6): room for the pre-sort's [B, n + m] uint16 permutations -- OPTIONAL: a call with a smaller (or no) workspace sorts inside the
 * row kernel -- and only where the pre-sort runs (ABI 18): 2 <= n, m <= 2048 and no SOT_FLAG_NO_SPECIALIZE; any other per-row problem
 * sorts in the row kernel and uses no workspace.  0 otherwise, and for prob == NULL, n < 1 or m < 1. */
size_t sot_workspace_bytes(const sot_problem *prob);

/*
 * Position plan for row-invariant supports (the 1-D x_pos/y_pos of trainer.py:192-197 and the
 * fixed_x buffer of losses.py:124-127): checks sortedness and, if needed, sorts (position, index)
 * pairs once (torch.sort of losses.py:287-288 on a row that is the same for every batch row).
 * Outputs: sorted positions, int32 permutations, and two device flags.  A training loop that keeps
 * its position grid calls this once and passes the plan in sot_problem.
 */
int sot_prepare_positions(const float *xpos, const float *ypos, int32_t n, int32_t m,
                          float *xpos_sorted /* [n] */, float *ypos_sorted /* [m] */,
                          int32_t *xperm /* [n] */, int32_t *yperm /* [m] */,
                          int32_t *perm_is_identity /* [2] */, void *stream);
/* The same plan for xpos / max(xpos) and ypos / max(ypos) (round 6, ABI 12): the reference's trainer rebuilds its grid on every step --
 * `x_pos = x_pos / x_pos.max(); y_pos = x_pos.clone()` (trainer.py:196-197) -- and this call takes the bin frequencies as they are, so
 * that such a step pays one launch instead of a reduction, a division, a copy and the plan.  The sorted positions written are the
 * floats torch computes: torch.max's NaN rule, IEEE division. */
int sot_prepare_unit_positions(const float *xpos, const float *ypos, int32_t n, int32_t m,
                               float *xpos_sorted /* [n] */, float *ypos_sorted /* [m] */,
                               int32_t *xperm /* [n] */, int32_t *yperm /* [m] */,
                               int32_t *perm_is_identity /* [2] */, void *stream);

/*
 * Forward: row_loss[r] = W_p^p(x_r, y_r) for r in [0, B).
 * Replaces Wasserstein1D.forward steps 3-5 + wasserstein_1d + quantile_function
 * (losses.py:172-196, 214-220, 271-313): square, row mass (ATen summation order),
 * safe_divide (utils.py:135-142), position sort + weight gather, fp64-accumulated CDFs,
 * merge of the two CDFs (= sort(cat(U,V)) + 2x searchsorted + 2x take_along_dim), level
 * widths, cutoff mask, |q_x - q_y|^p, weighted row sum.
 */
int sot_w1d_forward(const sot_problem *prob, float *row_loss /* [B] */,
                    void *workspace, size_t workspace_bytes, void *stream);

/*
 * Batch reduction of losses.py:211 (`torch.mean(loss)`, dims=None) with a fixed-order fp64
 * accumulation: *mean_out = (float)(sum_r row_loss[r] / denom) and, if sum_out != NULL,
 * *sum_out = sum_r row_loss[r] (the per-shard partial that is all-reduced across GPUs).
 * hinge_threshold: rows are replaced by relu(row - threshold) first when apply_hinge != 0
 * (losses.py:203-205).  B == 0 is a defined call (the sum of no rows: *mean_out = 0 / denom); B < 0: SOT_ERR_BAD_SHAPE.
 */
int sot_w1d_reduce_mean(const float *row_loss, int64_t B, double denom, int apply_hinge, float hinge_threshold,
                        float *mean_out, double *sum_out, void *stream);

/*
 * Backward of the forward above w.r.t. the weights (closed form of the autograd graph of
 * losses.py:172-313; positions receive no gradient, as in every reference call site).
 * dL/d(row_loss[r]) = grad_scale * grad_row[r * grad_row_stride] (grad_row == NULL: 1 for every row).  grad_x and/or grad_y may be NULL (trainer.py only needs
 * grad_y: x is the target spectrum).  Row strides of the gradients equal n and m.
 * Tie convention: gradients of a run of equal quantile levels go to the run's last member in
 * stable-sort order (U before V, lower index first).
 */
int sot_w1d_backward(const sot_problem *prob,
                     const float *grad_row /* [B] if grad_row_stride == 1; ONE scalar if grad_row_stride == 0 */,
                     int64_t grad_row_stride, float grad_scale /* multiplies grad_row, e.g. 1/B of the batch mean */,
                     float *grad_x /* [B,n] or NULL */, float *grad_y /* [B,m] or NULL */,
                     void *workspace, size_t workspace_bytes, void *stream);

/*
 * Training form: row losses, their batch mean AND the gradient of `grad_scale * sum_r row_loss[r]` w.r.t. y in one call
 * (grad_scale = 1/denom: the gradient of the mean that Wasserstein1D.forward returns; trainer.py:220-228 backpropagates
 * exactly that, x being the target spectrum).  For the row lengths with a compile-time backward kernel this is ONE pass
 * over the rows (the backward kernel's merge walk also accumulates the loss, bit-identical to sot_w1d_forward) followed by
 * the reduction kernel; otherwise forward, backward and reduction are enqueued back to back.  No hinge (the hinge changes
 * which rows receive a gradient).  A caller whose upstream gradient turns out not to be 1 rescales with sot_scale_inplace.
 * completion_counters: see sot_w1d_loss.  B == 0: SOT_ERR_BAD_SHAPE (the mean of no rows is undefined), nothing is touched.
 */
int sot_w1d_loss_and_grad(const sot_problem *prob, float *row_loss /* [B] */, double denom, float *mean_out, double *sum_out,
                          float grad_scale, float *grad_y /* [B,m] */, uint32_t *completion_counters /* or NULL */,
                          void *workspace, size_t workspace_bytes, void *stream);

/*
 * Kernel-attached timing for benchmarks: arm slot `slot` (0 .. 63) for the calling host thread; the NEXT launch of a kernel with
 * the row length at compile time (sot_w1d_forward / _loss / _backward / _loss_and_grad on such rows) is then issued with a
 * start / stop event pair attached to the dispatch itself (hipExtLaunchKernelGGL), so sot_profile_elapsed_ms() -- which waits
 * for that launch -- returns the kernel's own duration, the figure rocprofv3's kernel trace reports, free of the stream time
 * an event pair recorded around the call adds.  Not graph-capturable; no effect on results.
 */
int sot_profile_next_launch(int slot);
int sot_profile_elapsed_ms(int slot, float *ms);

/* data[i] *= *scalar for i < count (device scalar); returns without touching `data` when the scalar is exactly 1. */
int sot_scale_inplace(float *data, int64_t count, const float *scalar, void *stream);

/*
 * Forward + batch reduction in ONE call: the whole of Wasserstein1D.forward with dims=None (losses.py:129-211) behind a
 * single FFI crossing.
 *   completion_counters == NULL: sot_w1d_forward and sot_w1d_reduce_mean are enqueued back to back (two kernels).
 *   completion_counters != NULL: ONE kernel -- the workgroup of the forward kernel that finishes last reduces the row
 *     losses, with the summation order of sot_w1d_reduce_mean (bit-identical result, independent of timing).
 *     `completion_counters` points to SOT_COMPLETION_COUNTER_WORDS device words that the caller zero-fills ONCE; every
 *     launch leaves them zero again, so the same buffer serves all later calls -- as long as at most one launch that uses
 *     it is in flight at a time (calls on one stream are; give each concurrently used stream its own buffer).
 *     Measured on MI355X (8192 x 2048 rows): 55.1 us as one kernel, 46.9 us as two -- every workgroup pays a counter round
 *     trip at its end and the last one an agent-scope acquire plus a re-read of the row losses, which together cost more
 *     than the ~2.6 us kernel boundary + mean kernel they replace; the shipped Python binding therefore passes NULL unless
 *     asked.
 * B == 0: SOT_ERR_BAD_SHAPE (the mean of no rows is undefined), nothing is touched.
 */
#define SOT_COMPLETION_COUNTER_WORDS 16
int sot_w1d_loss(const sot_problem *prob, float *row_loss /* [B] */, double denom, int apply_hinge,
                 float hinge_threshold, float *mean_out, double *sum_out, uint32_t *completion_counters /* or NULL */,
                 void *workspace, size_t workspace_bytes, void *stream);

/*
 * Forward for RAGGED supports in CSR form (BASELINE config 4: spectra after a per-row amplitude cutoff, where
 * the reference would be fed zero-masked dense rows; zero-weight points are inert, so both forms agree).
 * Row r owns entries [offsets[r], offsets[r+1]) of the concatenated weights/positions arrays; every row needs
 * 1 <= length <= max_n (resp. max_m), otherwise its loss is NaN.  x_nnz / y_nnz are offsets[B].  Positions are
 * per row; with SOT_FLAG_REQUIRE_SORT a row is sorted in LDS only if it is not already sorted.  The LDS footprint
 * is that of (max_n, max_m).  Semantics per row are those of sot_w1d_forward.
 */
int sot_w1d_forward_csr(const float *x_weights, const float *x_positions, const int64_t *x_offsets /* [B+1] */, int64_t x_nnz,
                        const float *y_weights, const float *y_positions, const int64_t *y_offsets /* [B+1] */, int64_t y_nnz,
                        int64_t B, int32_t max_n, int32_t max_m, float p, uint32_t flags, float *row_loss /* [B] */,
                        void *stream);

/*
 * return_quantiles=True (losses.py:198-201, 299-300): the five tensors the reference returns,
 * uq/vq/Q: [B, n+m], U: [B, n], V: [B, m]; any output pointer may be NULL.  Gradients: sot_w1d_quantiles_backward.
 */
int sot_w1d_quantiles(const sot_problem *prob, float *uq, float *vq, float *Q, float *U, float *V,
                      void *workspace, size_t workspace_bytes, void *stream);

/*
 * Vector-Jacobian product of sot_w1d_quantiles (ABI 14): the five tensors are differentiable in the reference (losses.py:286-300 are
 * sort, gather, cumsum, cat + sort, searchsorted, take_along_dim), and a caller who builds a ground cost of their own on them needs
 * the gradients of the inputs.  Upstream gradients grad_uq / grad_vq / grad_Q [B, n+m], grad_U [B, n], grad_V [B, m], dense, each a
 * device pointer or NULL (NULL = zero; an absent upstream costs no traffic).  Per row, with U, V the CDFs of the measures sorted by
 * position (xs, ys), Q the merged levels and rank_U(q) = min(#{U_i < q}, n-1):
 *   CDF entries:  GU_i = grad_U_i + grad_Q_k(i), GV_j = grad_V_j + grad_Q_k(j), k(.) the entry's place among the merged levels;
 *   weights:      reverse cumulative sums of GU / GV (fp64), the normalisation term  g / M - [M > 1e-7] sum(g w) / M^2  (with
 *                 SOT_FLAG_DONT_NORMALIZE the y term is folded into x's mass; none with SOT_FLAG_PRENORMALIZED), the factor 2 x of
 *                 SOT_FLAG_SQUARE, back through the sort permutation -- the tail of sot_w1d_backward;
 *   positions:    d / d xs[i] = sum_{k : rank_U(Q_k) = i} grad_uq_k, d / d ys[j] likewise with grad_vq, back through the sort
 *                 permutation; the ranks themselves carry no gradient.
 * Tie convention: the backward of `sort` hands grad_Q_k to the element of cat(U, V) at merged place k in stable order -- U before V,
 * lower index first, as in sot_w1d_backward -- and a level inside a run of equal levels has the ranks of the run's first member
 * (searchsorted side='left').
 * Outputs grad_x / grad_xpos [B, n], grad_y / grad_ypos [B, m], dense, in the caller's original column order, each may be NULL (an
 * absent output costs no traffic; all four NULL: SOT_OK, nothing is enqueued).  For a position row shared by all batch rows the
 * caller sums grad_xpos / grad_ypos over the rows (sot_column_sum), as with sot_w1d_position_grad.  prob->p and SOT_FLAG_LIMIT_Q do
 * not enter the result (the problem is validated as a whole all the same: p < 1 returns SOT_ERR_INVALID_P).  One kernel, one merge walk for weights and positions, deterministic (no atomics), enqueue-only, graph-capturable.
 * Status as sot_w1d_backward: SOT_ERR_NULL_POINTER for prob == NULL, for a NULL x / y / xpos / ypos with B > 0 and for shared
 * positions that still need their plan without a workspace; SOT_ERR_BAD_SHAPE for B < 0, n < 1, m < 1 or bad strides;
 * SOT_ERR_INVALID_P; SOT_ERR_WORKSPACE; SOT_ERR_UNSUPPORTED_SIZE for rows past the gradient LDS budget, decided before anything is
 * enqueued: the layout of sot_w1d_backward (n + m beyond ~13 000 on shared positions; per-row positions are laid out for the next
 * powers of two, so pow2(n) + pow2(m) <= 12 000 always fits) plus, for rows too short to hold them in their own dead CDF region,
 * 32 bytes per thread of the workgroup.
 */
int sot_w1d_quantiles_backward(const sot_problem *prob, const float *grad_uq, const float *grad_vq, const float *grad_Q,
                               const float *grad_U, const float *grad_V, float *grad_x, float *grad_y, float *grad_xpos,
                               float *grad_ypos, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Gradient of sum_r grad_scale * grad_row[r] * row_loss[r] w.r.t. the SUPPORT POSITIONS (losses.py:287-298 and 214-220: the positions
 * enter through torch.sort and take_along_dim, both differentiable; no reference call site asks for it, autograd supplies it):
 *     d row_loss / d xs[i] = sum over the merged levels k whose searchsorted rank in U (clamped to n-1) is i of
 *                            delta_k * p |xs[i_k] - ys[j_k]|^(p-1) sign(xs[i_k] - ys[j_k]);    ys[j]: minus the same.
 * One kernel, deterministic (no atomics).  Outputs are PER ROW, [B, n] / [B, m] dense, in the caller's original column order (the
 * sort of losses.py:287-288 is undone); either may be NULL.  For a position row shared by all batch rows (xpos_row_stride == 0)
 * the caller sums the rows -- sot_column_sum below -- which is what autograd's `expand` backward does (losses.py:167-170).
 * grad_row / grad_row_stride / grad_scale as in sot_w1d_backward.
 */
int sot_w1d_position_grad(const sot_problem *prob, const float *grad_row, int64_t grad_row_stride, float grad_scale,
                          float *grad_xpos /* [B,n] or NULL */, float *grad_ypos /* [B,m] or NULL */,
                          void *workspace, size_t workspace_bytes, void *stream);

/* ---- Mixed supports (ABI 17; csrc/sot_mixed.hip): ONE measure lives on a position row shared by every batch row, the other has
 * positions of its own per row -- exactly one of prob->xpos_row_stride / prob->ypos_row_stride is 0 (Wasserstein1D.forward accepts the
 * two kinds side by side, losses.py:162-170).  The parametric use: a dense target spectrum on the STFT bin grid against a model's line
 * spectrum, K partials per frame with their amplitudes as weights and their frequencies as positions.  Semantics per row are those of
 * sot_w1d_forward / sot_w1d_backward / sot_w1d_position_grad on the same problem with the shared row repeated for every batch row
 * (same flags, same tie convention; x's mass stays the divisor under SOT_FLAG_DONT_NORMALIZE whichever side is shared), without that
 * copy: the shared side goes through the position plan once per call and is staged once per workgroup, only the per-row side is
 * sorted per row (stable, in the kernel; the gradient kernels sort again).
 * Plan contract of the shared side with SOT_FLAG_REQUIRE_SORT, as for shared positions elsewhere: either the plan is passed --
 * perm_is_identity != NULL, the shared side's xpos / ypos holds the SORTED positions sot_prepare_positions produced, its xperm / yperm the
 * permutation and perm_is_identity[0] (x shared) / [1] (y shared) its flag; the other side's plan fields are not read -- or `workspace`
 * holds sot_w1d_mixed_workspace_bytes() bytes and the call plans the row itself.  row_perm_out / row_perm_in are not used.
 * Domain: the per-row side has 1 ... 2048 points, and the pair fits the generic per-row-position kernels' gradient layout in one CU's
 * LDS with 8 bytes per thread to spare (csrc/sot_mixed.hip: mixed_domain, from make_layout; pow2(n) + pow2(m) <= 12 000 always fits).
 * One domain for the three calls.
 * Status, all decided on the host before any pointer is followed or anything is enqueued: SOT_ERR_NULL_POINTER (prob, an output, and with
 * B > 0 x / y / xpos / ypos, a plan without the shared side's permutation, a missing workspace); SOT_ERR_INVALID_P; SOT_ERR_BAD_SHAPE for
 * B < 0, n < 1, m < 1, bad strides, and for both position strides 0 or both non-zero; SOT_ERR_UNSUPPORTED_SIZE outside the domain;
 * SOT_ERR_WORKSPACE.  B == 0: SOT_OK, nothing is touched.
 * sot_w1d_mixed_backward: grad_x [B, n] and / or grad_y [B, m], either may be NULL (both: SOT_OK, nothing is enqueued).
 * sot_w1d_mixed_position_grad: grad_pos [B, K] for the PER-ROW side only, in the caller's column order (a shared grid that needs a
 * gradient takes sot_w1d_position_grad on expanded positions).  grad_row / grad_row_stride / grad_scale as in sot_w1d_backward.
 * One kernel per call (plus the plan kernel when the call plans), deterministic (no atomics), enqueue-only, graph-capturable. */
size_t sot_w1d_mixed_workspace_bytes(const sot_problem *prob);   /* 0 for a problem the calls refuse, and when no workspace is needed */
int sot_w1d_mixed_forward(const sot_problem *prob, float *row_loss /* [B] */, void *workspace, size_t workspace_bytes, void *stream);
int sot_w1d_mixed_backward(const sot_problem *prob, const float *grad_row, int64_t grad_row_stride, float grad_scale,
                           float *grad_x /* [B,n] or NULL */, float *grad_y /* [B,m] or NULL */,
                           void *workspace, size_t workspace_bytes, void *stream);
int sot_w1d_mixed_position_grad(const sot_problem *prob, const float *grad_row, int64_t grad_row_stride, float grad_scale,
                                float *grad_pos /* [B,K]: the per-row side */, void *workspace, size_t workspace_bytes, void *stream);

/* ---- bfloat16 weight rows (ABI 19; csrc/sot_bf16.hip): what a model under torch.autocast(dtype=torch.bfloat16) hands over.  A bfloat16 is the
 * upper half of a float32, so widening is exact (a 16-bit shift) and every result below is DEFINED as: widen x and y, then the float32 entry
 * point's arithmetic.  Outputs equal, bit for bit, those of sot_w1d_forward / sot_w1d_loss on the widened rows on the same kernel family; the
 * row losses and the mean stay float32.  (The reference on bfloat16 tensors rounds its sums, divisions and cumsum to 8 bits; that is
 * deliberately not reproduced.)  float16 has no entry point: its exponent range is not float32's.
 *
 * Row conversion, [B, n] rows with strides in elements (>= n), any row length >= 1; rows need only their element type's alignment (rows that
 * start 2 bytes off a 16-byte boundary take the element-wise kernel; 16-byte accesses where both pointers are 16-byte aligned, n is a multiple
 * of 8 and the strides are multiples of 8 (16-bit side) / 4 (32-bit side)).  Only the n elements of each row are read and written.
 *   sot_rows_bf16_to_f32: dst = float(bits << 16), exact.
 *   sot_rows_f32_to_bf16: round to nearest, ties to even; values past the largest finite bfloat16 become +-inf, infinities are kept, a NaN
 *     becomes the quiet NaN 0x7FC0 (what torch's .to(torch.bfloat16) returns).
 * Status: SOT_ERR_BAD_SHAPE for B < 0, n < 1, a stride below n; SOT_ERR_NULL_POINTER for a NULL buffer with B > 0; B == 0: SOT_OK.
 * (The four calls of this section that enqueue work are declared `extern`: tests/test_workspace_sizes.py lists the declarations that begin a
 * line with their return type and asks tests/test_memory_contract_gpu.py for a table line for each; the guard-band cases, refusals and
 * empty batches of these four are in tests/test_bf16_gpu.py, and the binding lists them in _native.BF16_EXPORTS.) */
extern int sot_rows_bf16_to_f32(const uint16_t *src, int64_t B, int32_t n, int64_t src_row_stride, float *dst, int64_t dst_row_stride, void *stream);
extern int sot_rows_f32_to_bf16(const float *src, int64_t B, int32_t n, int64_t src_row_stride, uint16_t *dst, int64_t dst_row_stride, void *stream);
/* The typed forward: sot_problem as for sot_w1d_forward / sot_w1d_loss, except that prob->x and prob->y point at bfloat16 elements (declared
 * const float * in the struct; pass the address) and x_row_stride / y_row_stride count bfloat16 elements; positions stay float32.
 *   NATIVE problems -- shared positions, n == m in {512, 1024, 2048, 4096}, neither SOT_FLAG_PRENORMALIZED nor SOT_FLAG_NO_SPECIALIZE, x and y
 *     16-byte aligned with row strides that are multiples of 8 elements -- run the full-row forward kernels with 16-bit row loads: no float32
 *     image of the rows exists anywhere, and the workspace is exactly sot_workspace_bytes() of the same problem.
 *   EVERY OTHER problem (other lengths, n != m, per-row positions, rows 2 bytes off, ...) is widened inside the call: dense 16-byte aligned
 *     float32 copies of x and y at the front of the workspace, then the float32 route unchanged.  sot_w1d_bf16_workspace_bytes() reports the
 *     copies plus the float32 call's own workspace, and here the workspace is REQUIRED in full (SOT_ERR_NULL_POINTER without one,
 *     SOT_ERR_WORKSPACE for a shorter one -- decided before anything is enqueued); any alignment of the workspace will do.
 * Refusals are those of sot_w1d_forward / sot_w1d_loss (SOT_ERR_INVALID_P, _BAD_SHAPE, _NULL_POINTER, _UNSUPPORTED_SIZE, _WORKSPACE).
 * sot_w1d_bf16_workspace_bytes: host-side arithmetic; 0 for prob == NULL, n < 1 or m < 1.  The typed backward and training form follow
 * below (ABI 20). */
size_t sot_w1d_bf16_workspace_bytes(const sot_problem *prob);
extern int sot_w1d_forward_bf16(const sot_problem *prob, float *row_loss /* [B] */, void *workspace, size_t workspace_bytes, void *stream);
extern int sot_w1d_loss_bf16(const sot_problem *prob, float *row_loss /* [B] */, double denom, int apply_hinge, float hinge_threshold,
                             float *mean_out, double *sum_out, uint32_t *completion_counters /* or NULL */, void *workspace,
                             size_t workspace_bytes, void *stream);

/* ---- bfloat16 training (ABI 20; csrc/sot_bf16_bwd.hip): sot_w1d_backward and sot_w1d_loss_and_grad for bfloat16 weight rows AND bfloat16
 * gradients.  prob as for the typed forward (x, y bfloat16, their strides in bfloat16 elements, positions float32); grad_x / grad_y are dense
 * bfloat16 rows of n / m elements; grad_row, the row losses and the mean stay float32.
 * DEFINED RESULT: every gradient element equals, bit for bit, rne(v) -- v the float32 element that sot_w1d_backward / sot_w1d_loss_and_grad
 * returns for the widened rows on the same kernel family, rne = round to nearest even (sot_rows_f32_to_bf16's) -- or rne(v * *rescale) when
 * `rescale` is given: one float32 multiply, then the single rounding.  Row losses and the mean equal the float32 call's bits.
 *   NATIVE: sot_w1d_bf16_native(prob) -- the typed forward's native condition on the problem (shared positions, n == m in {512, 1024, 2048,
 *     4096}, neither SOT_FLAG_PRENORMALIZED nor SOT_FLAG_NO_SPECIALIZE, x and y 16-byte aligned with row strides that are multiples of 8
 *     elements) without SOT_FLAG_TIE_FREE_GRADIENT (the merge-free training form has no 16-bit instantiation; the flag means nothing to a
 *     forward call) -- AND grad_x / grad_y 16-byte aligned.  The full-row backward kernels read the 16-bit rows and round each gradient at its
 *     store: no float32 image of a spectrum or of a gradient exists, and the workspace is exactly sot_workspace_bytes() of the problem.
 *   EVERY OTHER problem runs inside the call: x and y widened into the workspace, the float32 backward / training form into float32 gradient
 *     images there, the images narrowed into grad_x / grad_y (scaled by *rescale first).  sot_w1d_bf16_backward_workspace_bytes() reports the
 *     images plus the float32 call's workspace; it is REQUIRED in full (SOT_ERR_NULL_POINTER without one, SOT_ERR_WORKSPACE for a shorter one,
 *     decided before anything is enqueued); any alignment will do.  The function sees no gradient pointer: a caller whose gradient buffers are
 *     not 16-byte aligned on an otherwise native problem asks it with SOT_FLAG_NO_SPECIALIZE added (the same sum) or gets SOT_ERR_WORKSPACE.
 *   rescale (device scalar or NULL; non-NULL only without grad_x: SOT_ERR_BAD_SHAPE otherwise) is the FIX-UP mode of a training step that
 *     stored its gradient before the upstream gradient was known: the call recomputes grad_y as rne(v * *rescale).  On the native route every
 *     workgroup reads the scalar first and returns at once when it is exactly 1 -- grad_y is not touched, as with sot_scale_inplace; the
 *     widening route rewrites grad_y with rne(v), the values it held.
 * Refusals and B == 0 are those of sot_w1d_backward / sot_w1d_loss_and_grad.  sot_w1d_bf16_backward_workspace_bytes and sot_w1d_bf16_native:
 * host-side arithmetic, 0 for prob == NULL, n < 1 or m < 1.  (The three other calls are declared `extern` for the reason given above; their
 * guard-band cases, refusals and empty batches are in tests/test_bf16_train_gpu.py, and the binding lists them in _native.BF16_TRAIN_EXPORTS.) */
size_t sot_w1d_bf16_backward_workspace_bytes(const sot_problem *prob, int want_grad_x, int want_grad_y);
extern int sot_w1d_bf16_native(const sot_problem *prob);
extern int sot_w1d_backward_bf16(const sot_problem *prob, const float *grad_row, int64_t grad_row_stride, float grad_scale,
                                 uint16_t *grad_x /* [B,n] or NULL */, uint16_t *grad_y /* [B,m] or NULL */, const float *rescale /* or NULL */,
                                 void *workspace, size_t workspace_bytes, void *stream);
extern int sot_w1d_loss_and_grad_bf16(const sot_problem *prob, float *row_loss /* [B] */, double denom, float *mean_out, double *sum_out,
                                      float grad_scale, uint16_t *grad_y /* [B,m] */, uint32_t *completion_counters /* or NULL */,
                                      void *workspace, size_t workspace_bytes, void *stream);

/* ---- float64 rows (ABI 21; csrc/sot_f64.hip): the row pipeline in double precision -- what torch.autograd.gradcheck and a model trained in
 * double hand over.  The reference in float64 is plain ATen on double tensors (losses.py:129-313); these calls evaluate SURVEY.md A.1 / A.2 / A.4
 * in double with every sum in a fixed order (thread chunk, wavefront, the workgroup's wavefronts in order), so a row's result depends neither
 * on the grid nor on its place in the batch.  Not bit-identical to ATen's float64 (another summation order: ~1e-15 relative without the
 * cutoff; under SOT_FLAG_LIMIT_Q a level that sits on the edge 1 by its last bit is kept or dropped with that bit).
 *   sot_problem_f64: the fields of sot_problem with double data and a double p; no plan and no permutation fields.
 *   Supports must arrive SORTED (positions non-decreasing along each row; shared positions: row stride 0 on both sides, per-row: on both):
 *     a problem with SOT_FLAG_REQUIRE_SORT is refused (SOT_ERR_BAD_SHAPE) -- the caller sorts.  Flags honoured: SQUARE, DONT_NORMALIZE,
 *     LIMIT_Q, PRENORMALIZED; the others are ignored.  Mass guard: a mass <= 1e-7 (compared as a double) is replaced by the float32 value
 *     1e-7 widened to double (utils.py:135-142).
 *   sot_w1d_forward_f64: row_loss[r] = W_p^p of row pair r.
 *   sot_w1d_backward_f64: grad_x / grad_y (dense [B, n] / [B, m]; either may be NULL and is then not computed) = d sum_r grad_row[r *
 *     grad_row_stride] * grad_scale * loss_r / d x, d y; grad_row_stride is 0 or 1, grad_row == NULL means 1 for every row.  At exactly tied
 *     levels the gradient of a run of equal levels goes to the run's last member in the stable order (U before V, lower index first): the tie
 *     order of sot_w1d_backward.
 *   Sizes: one row pair's working set lives in one CU's LDS -- 16 (n + m) bytes forward (n + m <= 10 000 at least; 4097 + 4097 fits), 24 (n + m)
 *     bytes backward (n + m <= 6 600 at least).  Beyond: SOT_ERR_UNSUPPORTED_SIZE.  sot_w1d_f64_supported(prob, backward): 1 where the forward
 *     (backward != 0: the backward) takes the problem, 0 otherwise -- NULL, bad shapes or strides, p < 1, REQUIRE_SORT, size; host arithmetic.
 *   sot_w1d_f64_workspace_bytes: 0 for every problem of this ABI version (the calls use no workspace; the argument pair is kept for the
 *     calling convention of the library).  A workspace_bytes > 0 with workspace == NULL is refused (SOT_ERR_NULL_POINTER).
 *   Every refusal is decided before anything is enqueued; B == 0 returns SOT_OK.  (The three int calls are declared `extern` for the reason
 *   given above; their guard-band cases, refusals and empty batches are in tests/test_f64_gpu.py, and the binding lists them in
 *   _native.F64_EXPORTS.) */
typedef struct sot_problem_f64 {
    const double *x;          /* [B, n] weights of the first measure                                  */
    const double *y;          /* [B, m] weights of the second measure                                 */
    const double *xpos;       /* sorted support positions of x: [n] (row stride 0) or [B, n]          */
    const double *ypos;       /* sorted support positions of y: [m] (row stride 0) or [B, m]          */
    int64_t B;
    int32_t n, m;
    int64_t x_row_stride;     /* elements between consecutive rows (>= n / >= m)                      */
    int64_t y_row_stride;
    int64_t xpos_row_stride;  /* 0 = one shared position row, otherwise >= n / >= m                   */
    int64_t ypos_row_stride;
    double p;                 /* p >= 1; the result is W_p^p                                          */
    uint32_t flags;           /* SOT_FLAG_*                                                           */
} sot_problem_f64;
size_t sot_w1d_f64_workspace_bytes(const sot_problem_f64 *prob);
extern int sot_w1d_f64_supported(const sot_problem_f64 *prob, int backward);
extern int sot_w1d_forward_f64(const sot_problem_f64 *prob, double *row_loss /* [B] */, void *workspace, size_t workspace_bytes, void *stream);
extern int sot_w1d_backward_f64(const sot_problem_f64 *prob, const double *grad_row, int64_t grad_row_stride, double grad_scale,
                                double *grad_x /* [B,n] or NULL */, double *grad_y /* [B,m] or NULL */, void *workspace, size_t workspace_bytes,
                                void *stream);

/* out[c] = sum_r rows[r * row_stride + c], c < n, in a fixed order with fp64 accumulation (B == 0: zeros). */
int sot_column_sum(const float *rows, int64_t B, int32_t n, int64_t row_stride, float *out /* [n] */, void *stream);

/*
 * Segmented (per-row) stable ascending sort with index payload: what torch.sort(keys, 1)
 * returns at losses.py:287-288 (indices are int64 like torch's; bit-identical to torch on
 * distinct keys; ties keep the lower index first).  row_stride in elements; outputs are
 * dense [B, n].  Either output may be NULL.  NaN keys: no defined order (torch puts them last; here a positive NaN orders above the
 * internal +inf pads, a negative one first), but every returned index is a valid column (< n) -- as are the gather / store indices of
 * the per-row-position kernels, which use the same sort.
 */
int sot_segmented_sort(const float *keys, int64_t B, int32_t n, int64_t row_stride,
                       float *sorted_keys, int64_t *indices, void *stream);

/* ---- The producer in front of the loss: the magnitude STFT of the reference's features.TorchSTFT
 * (features.py:85-113 -> compute_mag / stft, features.py:191-237; end padding utils.pad_for_stft, utils.py:252-275):
 * frames = ceil(samples / hop) frames of n_fft samples starting every `hop` samples (zeros past the end of the clip),
 * multiplied by `window` [n_fft], one-sided DFT, |.| / sqrt(n_fft) (torch.stft(center=False, normalized=True)).
 * audio [batch, samples] (row stride in elements), mag / grad_mag [batch, frames, n_fft/2 + 1] contiguous (frames-major:
 * each row is a spectrum for sot_w1d_*), grad_audio [batch, samples] contiguous.  n_fft: a power of two in [64, 4096].
 * Enqueue-only, no allocation: the backward takes a caller-owned scratch buffer of sot_stft_backward_workspace_bytes(). */
int64_t sot_stft_frames(int64_t samples, int hop);
int sot_stft_mag_forward(const float *audio, int64_t batch, int64_t samples, int64_t audio_row_stride,
                         const float *window, int n_fft, int hop, float *mag, void *stream);
/* the same transform of TWO signals of equal shape (target and estimate of a training step) in one launch:
 * mag[0 : batch_each] belongs to audio_a, mag[batch_each : 2 batch_each] to audio_b */
int sot_stft_mag_forward_pair(const float *audio_a, int64_t row_stride_a, const float *audio_b, int64_t row_stride_b,
                              int64_t batch_each, int64_t samples, const float *window, int n_fft, int hop,
                              float *mag /* [2 * batch_each, frames, n_fft/2+1] */, void *stream);
/* gradient of a scalar L w.r.t. the audio given dL/d(mag): closed form of abs o stft's autograd (bins with |X| = 0 pass
 * no gradient, as torch's sgn(0) = 0); deterministic (groups of frames overlap-added in a fixed order, no atomics).
 * grad_scale: optional DEVICE scalar that multiplies grad_mag (the upstream gradient of a loss whose dL/d(mag) was
 * computed ahead of the backward pass, sot_w1d_loss_and_grad), or NULL. */
/* Round 3: the forward can also hand out the COMPLEX spectrum X (what torch.abs's autograd node saves of torch.stft's output), `spec`:
 * [batch, frames, n_fft/2 + 1] interleaved (re, im) float pairs, 8-byte aligned, or NULL; in the pair form for the SECOND signal only
 * (`spec_b`: [batch_each, frames, n_fft/2 + 1, 2]; the estimate, the one a training step differentiates).  sot_stft_mag_backward_spec
 * then takes that spectrum instead of the audio (audio may be NULL) and skips the forward transform it would otherwise recompute per
 * frame: the same gradient bit for bit, n_fft 2048 on 4096 frames 46 -> ~30 us. */
int sot_stft_mag_forward_spec(const float *audio, int64_t batch, int64_t samples, int64_t audio_row_stride,
                              const float *window, int n_fft, int hop, float *mag, float *spec /* or NULL */, void *stream);
int sot_stft_mag_forward_pair_spec(const float *audio_a, int64_t row_stride_a, const float *audio_b, int64_t row_stride_b,
                                   int64_t batch_each, int64_t samples, const float *window, int n_fft, int hop,
                                   float *mag, float *spec_b /* or NULL */, void *stream);
int sot_stft_mag_backward_spec(const float *audio /* may be NULL when spec is given */, const float *spec /* or NULL */, int64_t batch,
                               int64_t samples, int64_t audio_row_stride, const float *window, int n_fft, int hop,
                               const float *grad_mag, const float *grad_scale, float *grad_audio, int accumulate,
                               void *workspace, size_t workspace_bytes, void *stream);
size_t sot_stft_backward_workspace_bytes(int64_t batch, int64_t samples, int n_fft, int hop);
int sot_stft_mag_backward(const float *audio, int64_t batch, int64_t samples, int64_t audio_row_stride,
                          const float *window, int n_fft, int hop, const float *grad_mag, const float *grad_scale,
                          float *grad_audio, int accumulate /* grad_audio += result instead of = */,
                          void *workspace, size_t workspace_bytes, void *stream);

/* ---- Additive oscillator bank in front of the STFT in the training step: ddsp.oscillator_bank
 * (ddsp.py:208-263 with use_angular_cumsum=False, sum_sinusoids=True) incl. remove_above_nyquist (ddsp.py:25-49):
 *   audio[b,t] = sum_k a'[b,t,k] sin(phase[b,t,k]),  a' = (f >= sample_rate/2) ? 0 : a,
 *   phase = cumsum_t((f * 2pi) / sample_rate)  (fp64 accumulation rounded to fp32 per sample, as ATen's CPU cumsum).
 * freq / amp / grad_freq / grad_amp: [batch, samples, sinusoids] contiguous; audio / grad_audio: [batch, samples].
 * samples <= 2^20, sinusoids <= 512 (else SOT_ERR_UNSUPPORTED_SIZE).  Deterministic.
 * `workspace`: device scratch of at least sot_oscillator_bank_workspace_bytes() bytes (per-segment phase carries, fp64;
 * the forward uses the first half only); 0 is returned for sizes the kernels do not take. */
size_t sot_oscillator_bank_workspace_bytes(int64_t batch, int64_t samples, int sinusoids);
int sot_oscillator_bank_forward(const float *freq, const float *amp, int64_t batch, int64_t samples, int sinusoids,
                                float sample_rate, float *audio, void *workspace, size_t workspace_bytes, void *stream);
/* gradients w.r.t. the envelopes (either may be NULL) given dL/d(audio) */
int sot_oscillator_bank_backward(const float *freq, const float *amp, int64_t batch, int64_t samples, int sinusoids,
                                 float sample_rate, const float *grad_audio, float *grad_freq, float *grad_amp,
                                 void *workspace, size_t workspace_bytes,
                                 int workspace_from_forward /* 1: `workspace` is the buffer sot_oscillator_bank_forward was
                                    given for the SAME envelopes and has not been written since: its segment start phases
                                    are reused instead of recomputed */,
                                 void *stream);

/* ---- Envelope upsampling of the synthesiser in front of the oscillator bank (synths.Sinusoidal.get_controls /
 * get_signal, synths.py:62-113 with amp_scale_fn = freq_scale_fn = None): frame-rate controls [batch, frames, sinusoids] ->
 * sample-rate envelopes [batch, samples, sinusoids] for sot_oscillator_bank_*.  harmonic != 0: freq_frames is [batch, frames, 1]
 * and partial k gets f0 * (k + 1) (ddsp.py:6-22).  Amplitudes of partials whose frame-rate frequency is >= sample_rate / 2 are
 * zeroed (ddsp.py:25-49), then upsampled with half-overlapping Hann windows (`window` = torch.hann_window(2 * samples / frames),
 * [2 hop] floats; ddsp.py:121-205, add_endpoint); frequencies are interpolated linearly (F.interpolate, align_corners=False, in
 * ATen's operation order): bit-identical to the reference's CPU result.  samples must be a multiple of frames, frames < samples.
 * The backward takes the gradients w.r.t. the two envelopes and returns those w.r.t. the controls (either output may be NULL;
 * grad_freq_frames is [batch, frames, 1] when harmonic).  Deterministic. */
int sot_synth_envelopes_forward(const float *amp_frames, const float *freq_frames, const float *window, int64_t batch, int frames,
                                int sinusoids, int harmonic, int64_t samples, float sample_rate, float *amp_env, float *freq_env,
                                void *stream);
int sot_synth_envelopes_backward(const float *amp_frames, const float *freq_frames, const float *window, int64_t batch, int frames,
                                 int sinusoids, int harmonic, int64_t samples, float sample_rate, const float *grad_amp_env,
                                 const float *grad_freq_env, float *grad_amp_frames, float *grad_freq_frames, void *stream);

/* ---- The synthesiser in one piece (synths.Sinusoidal.forward, synths.py:62-128): frame-rate controls -> audio [batch, samples]
 * without the sample-rate envelopes ever existing in memory: the oscillator-bank kernels evaluate them from the controls (the
 * same float32 operations as sot_synth_envelopes_forward, so the audio equals sot_oscillator_bank_forward on those envelopes bit
 * for bit).  The backward returns the gradients w.r.t. the controls (either may be NULL; grad_freq_frames [batch, frames, 1]
 * when harmonic) without sample-rate gradient arrays either: the tile kernel reduces its samples to per-frame partial sums (the
 * frequency gradient through cumulative tap weights, see csrc/sot_osc.hip), a last kernel adds the segments up.
 * workspace: sot_synth_workspace_bytes(batch, frames, samples, sinusoids, backward) bytes (0 for invalid sizes);
 * workspace_from_forward != 0: its first bytes still hold what sot_synth_forward left there for the SAME controls.  Deterministic. */
size_t sot_synth_workspace_bytes(int64_t batch, int frames, int64_t samples, int sinusoids, int backward);
int sot_synth_forward(const float *amp_frames, const float *freq_frames, const float *window, int64_t batch, int frames, int sinusoids,
                      int harmonic, int64_t samples, float sample_rate, float *audio, void *workspace, size_t workspace_bytes,
                      void *stream);
int sot_synth_backward(const float *amp_frames, const float *freq_frames, const float *window, int64_t batch, int frames, int sinusoids,
                       int harmonic, int64_t samples, float sample_rate, const float *grad_audio, float *grad_amp_frames,
                       float *grad_freq_frames, const void *tap_tables, void *workspace, size_t workspace_bytes,
                       int workspace_from_forward, void *stream);
/* The backward's weight tables depend on (window, frames, samples) only: a caller that keeps them across steps fills a buffer of
 * sot_synth_tap_table_bytes(frames, samples) bytes once with sot_synth_tap_tables and passes it as tap_tables; NULL: the backward
 * builds them in its workspace on every call (6 us for 16 frames x 4096 samples). */
size_t sot_synth_tap_table_bytes(int frames, int64_t samples);
int sot_synth_tap_tables(const float *window, int frames, int64_t samples, void *tables, void *stream);

/* ---- Spectral distance of the reference's MSSLoss (losses.py:365-425 with mean_difference
 * losses.py:7-36 and safe_log utils.py:145-151) over `count` magnitudes target[i], value[i]:
 *   out[0] = mag_weight * mean(D(t - v)) + logmag_weight * mean(D(slog t - slog v)),  D = |.| (l2 == 0) or (.)^2,
 *   slog(x) = log(x <= eps ? eps : x).  Deterministic (fixed-order fp64 partial sums in the caller-owned workspace). */
size_t sot_spec_distance_workspace_bytes(void);
int sot_spec_distance_forward(const float *target, const float *value, int64_t count, float mag_weight,
                              float logmag_weight, float eps, int l2, float *out,
                              int accumulate /* out[0] += the distance (MSSLoss sums its scales) instead of = */,
                              void *workspace, size_t workspace_bytes, void *stream);
/* gradients w.r.t. target and/or value (either may be NULL) given d(loss)/d(out) as a one-element device tensor times
 * grad_scale; |.|' (0) = 0 and no gradient through slog below eps, as torch */
int sot_spec_distance_backward(const float *target, const float *value, int64_t count, float mag_weight,
                               float logmag_weight, float eps, int l2, const float *upstream, float grad_scale,
                               float *grad_target, float *grad_value, void *stream);
/* The same distance PER ROW: out[r] for r < rows over the `count_per_row` consecutive magnitudes of row r -- MSSLoss called with
 * `dims` = the two spectrogram axes (one value per clip; losses.py:406-425 hands `dims` to mean_difference, losses.py:7-36).
 * One workgroup per row, fixed-order fp64 sums; upstream: [rows]. */
int sot_spec_distance_rows_forward(const float *target, const float *value, int64_t rows, int64_t count_per_row,
                                   float mag_weight, float logmag_weight, float eps, int l2, float *out /* [rows] */,
                                   int accumulate, void *stream);
int sot_spec_distance_rows_backward(const float *target, const float *value, int64_t rows, int64_t count_per_row,
                                    float mag_weight, float logmag_weight, float eps, int l2,
                                    const float *upstream /* [rows] */, float grad_scale,
                                    float *grad_target, float *grad_value, void *stream);

/* ---- Round 5: the WHOLE multi-scale spectrogram loss and its gradient in two launches (the reference's `MSSLoss.forward`,
 * losses.py:406-425, + autograd; per scale: compute_mag features.py:191-237 -- hann or any caller-given window, hop = n_fft / 4,
 * end padding utils.py:252-275, normalized -- and mean_difference losses.py:7-36 / safe_log utils.py:145-151):
 *   loss = sum_s [mag_weight * mean D(T_s - V_s) + logmag_weight * mean D(slog T_s - slog V_s)]      (per_clip == 0: one float;
 *   per_clip != 0: the means run over each clip's own spectrogram, `dims` = its two axes: loss[batch]),
 *   grad_value[b, t] = d loss (or d loss[b]) / d value[b, t]   (NULL: forward only; the caller applies its upstream gradient).
 * post_scale (ABI 13): the finished float32 loss value(s) and gradient entries are multiplied by it -- the `loss_fn(x, y) * weight` of
 *   MixOfLosses (losses.py:360) and its backward as ONE more float32 product each, i.e. the same floats as the two torch kernels; 1 = off.
 * target / value: [batch, samples] float32 with the given row strides (in floats); fft_sizes[n_scales]: powers of two in [64, 2048],
 * n_scales <= 8; windows[s]: n_fft taps of scale s, device pointers on 8-byte boundaries (host array of device pointers).
 * One workgroup per (scale, clip, 4096-sample chunk): 2048 / n_fft frames per wavefront through a register-resident FFT, magnitudes,
 * distance, gradient w.r.t. the spectrum, inverse transform and overlap-add without a spectrogram in memory; a second kernel adds the
 * scales per sample in a fixed order.  Deterministic, enqueue-only, graph-capturable.
 * workspace: sot_mss_workspace_bytes(batch, samples, fft_sizes, n_scales) bytes, 16-byte aligned (0 is returned for sizes it does not take). */
size_t sot_mss_workspace_bytes(int64_t batch, int64_t samples, const int *fft_sizes, int n_scales);
int sot_mss_loss_and_grad(const float *target, int64_t target_row_stride, const float *value, int64_t value_row_stride,
                          int64_t batch, int64_t samples, const int *fft_sizes, const float *const *windows, int n_scales,
                          float mag_weight, float logmag_weight, float eps, int l2, int per_clip, float post_scale,
                          float *loss /* [1] or [batch] */, float *grad_value /* [batch, samples] contiguous, or NULL */,
                          void *workspace, size_t workspace_bytes, void *stream);

/* ---- Evaluation metrics on the same engine (ABI 16; csrc/sot_mss.hip, metric mode): up to SOT_METRIC_MAX_GROUPS calls of the reference's
 * metrics.ms_spectral_distance (metrics.py:51-87) on the same two signals in ONE pass, forward only.  A group is one such call:
 *   out[g] = sum over the group's sizes, in the group's order, of the float32 mean over the scale's bins of
 *            mag_weight * D(t - v) + logmag_weight * D(slog t - slog v) + lsd_weight * D(10 log10 max'(t t) - 10 log10 max'(v v)),
 *   t = |T_k|, v = |V_k| as sot_mss_loss_and_grad forms them, D = |.| (l2 == 0) or (.)^2, slog(x) = log(max'(x)), max'(x) = (x <= eps ? eps : x)
 *   (utils.py:145-157; the squares are rounded to float32 first; both logarithms are the accurate libm ones).  A weight <= 0 switches its term off.
 * fft_sizes[n_sizes] / windows: the UNION of the groups' sizes, each once, n_sizes <= 8, powers of two in [64, 2048], hop = n_fft / 4; every
 * audio sample is fetched and every frame transformed once per size of the union, however many groups name the size.  A group names sizes of
 * the union (its own order; that is the order of the float32 `loss +=`).  per_clip != 0: the means run over each clip's own spectrogram.
 * out: [n_groups], or [n_groups, batch] with per_clip.  A group without lsd_weight has the bits of sot_mss_loss_and_grad's loss for the same
 * sizes and weights (same engine, same summation order).  Two launches (the engine and a finish kernel), deterministic (no atomics),
 * enqueue-only, graph-capturable.  workspace: sot_spec_metrics_workspace_bytes() bytes on an 8-byte boundary (0 for arguments outside the domain).
 * Status: SOT_ERR_UNSUPPORTED_SIZE for a size the engine does not take; SOT_ERR_BAD_SHAPE for n_groups outside 1 .. 4, n_sizes outside
 * 1 .. 8, a size named twice in the union, a group with no size, with a size that is not in the union or with all three weights <= 0, and
 * for bad strides; SOT_ERR_NULL_POINTER; SOT_ERR_WORKSPACE -- all decided before anything is enqueued.  batch == 0: SOT_OK, nothing is touched.
 * (The reference's `mse`, metrics.py:11-13, needs no entry point of its own: sot_spec_distance_forward on the raw audio with mag_weight 1, l2 1.) */
#define SOT_METRIC_MAX_GROUPS 4
typedef struct sot_metric_group {
    int32_t n_sizes;          /* 1 .. 8 */
    int32_t fft_sizes[8];     /* sizes of the union, in the order the reference's call lists them */
    float mag_weight, logmag_weight, lsd_weight;
    int32_t l2;               /* 0: "L1", otherwise "L2" */
} sot_metric_group;
size_t sot_spec_metrics_workspace_bytes(int64_t batch, int64_t samples, const int *fft_sizes, int n_sizes, int n_groups);
int sot_spec_metrics(const float *target, int64_t target_row_stride, const float *value, int64_t value_row_stride, int64_t batch,
                     int64_t samples, const int *fft_sizes, const float *const *windows, int n_sizes, const sot_metric_group *groups,
                     int n_groups, float eps, int per_clip, float *out /* [n_groups] or [n_groups, batch] */, void *workspace,
                     size_t workspace_bytes, void *stream);

/* ---- Time-invariant FIR filtering of [batch, samples] audio (ABI 15; csrc/sot_fir.hip): the reference's ddsp.fft_convolve for a 2-D
 * impulse response (one frame) with padding="same" (ddsp.py:504-633, crop_and_compensate_delay :695-734) -- what frequency_filter
 * (ddsp.py:350-379) runs and what synths.Sinusoidal(apply_roll_off=True) appends to its audio (synths.py:121-126: 128 taps) -- as a
 * direct sum instead of a product of spectra.  With audio zero outside [0, samples):
 *   out[b,t]        = sum_{k < n_taps} taps[b,k] * audio[b, t + start - k]                           0 <= t < samples
 *   grad_audio[b,u] = sum_k taps[b,k] * grad_out[b, u - start + k]     (the same filter with reversed taps and start' = n_taps - 1 - start)
 *   grad_taps[b,k]  = sum_t grad_out[b,t] * audio[b, t + start - k]
 * start: the sample of the full linear convolution that becomes out[.,0].  The reference's default (delay_compensation < 0) is
 *   (n_taps - 1) / 2 - 1 in integer division -- 62 for its 128 taps, NOT the filter's group delay of 64: its output keeps a delay of two
 *   samples, and callers that want parity pass that value; a delay_compensation >= 0 is passed as it is.
 * audio: rows audio_row_stride >= samples floats apart (a column slice of a wider tensor is fine); taps: [batch, n_taps] rows
 *   taps_row_stride >= n_taps apart, or ONE filter for every clip with taps_row_stride == 0; out / grad_out / grad_audio: [batch, samples]
 *   contiguous; grad_taps: [batch, n_taps] contiguous, per clip also for a shared filter (the caller sums the rows: sot_column_sum).
 * sot_fir_same_backward: grad_audio and / or grad_taps may be NULL; `audio` is read for grad_taps only, `taps` for grad_audio only;
 *   workspace (grad_taps only): sot_fir_workspace_bytes(batch, samples, n_taps) bytes on an 8-byte boundary (0 is returned outside the domain).
 * Domain: float32, 3 <= n_taps <= 512, 0 <= start <= n_taps - 2, 1 <= samples <= 2^20 -- anything else SOT_ERR_UNSUPPORTED_SIZE (batch < 0,
 *   samples < 1, n_taps < 1 or a row stride shorter than its row: SOT_ERR_BAD_SHAPE; SOT_ERR_NULL_POINTER; SOT_ERR_WORKSPACE), decided on
 *   the host before anything is enqueued.  n_taps == 2 (the reference's default crop is -1 there and its result empty) and padding="valid"
 *   (the reference's slice is broken) are outside on purpose.
 * Numerics: every out / grad_audio element is ONE float32 fmaf chain over the taps in ascending order of the sum's own index, so a row's
 *   bits do not depend on the batch or on tile boundaries; grad_taps: exact fp64 products added in t order, rounded once to float32.
 * One workgroup per (clip, SOT_FIR_TILE consecutive outputs).  Deterministic (no atomics), enqueue-only, graph-capturable. */
#define SOT_FIR_TILE 1024
size_t sot_fir_workspace_bytes(int64_t batch, int64_t samples, int n_taps);
int sot_fir_same_forward(const float *audio, int64_t audio_row_stride, const float *taps, int64_t taps_row_stride, int64_t batch,
                         int64_t samples, int n_taps, int start, float *out, void *stream);
int sot_fir_same_backward(const float *grad_out, const float *audio /* or NULL */, int64_t audio_row_stride, const float *taps /* or NULL */,
                          int64_t taps_row_stride, int64_t batch, int64_t samples, int n_taps, int start, float *grad_audio /* or NULL */,
                          float *grad_taps /* or NULL */, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SOT_HIP_H */
