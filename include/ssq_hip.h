/*
 * ssq_hip.h -- C-ABI of libssq_hip.so, the MI355X (gfx950) synchrosqueezing engine.
 *
 * This header is the drop-in boundary for the hot path of jesusdpa1/ssqueeze_rs:
 * each entry point replaces one PyO3 `#[pyfunction]` of the reference's `_rs`
 * extension module (registered at rust/src/lib.rs:22-35).  Plain pointers and
 * sizes only; no Python, no torch types.  All functions return 0 on success and
 * a non-zero status on failure; `ssq_last_error()` then holds a message
 * (thread-local).  The library never frees or retains caller memory.
 *
 * dtype: SSQ_F32 (float in, interleaved complex-float out) or SSQ_F64
 * (double in, interleaved complex-double out).  SSQ_F64 with batch == 1 is the
 * reference's own configuration (PyReadonlyArray1<f64> in, complex128 out).
 * Batches are C-contiguous `[batch][N]` in and `[batch][rows][cols]` out.
 *
 * Two families:
 *   *_host  : host pointers in/out (H2D, kernels, D2H inside) -- what the
 *             Python/NumPy mirror `ssqueeze_rs_amd._rs` binds.
 *   plans   : device pointers + a caller stream, no allocation and no host
 *             synchronisation in the exec call (hipGraph-capturable) -- what
 *             batch pipelines and bench.py bind.
 */
#ifndef SSQ_HIP_H
#define SSQ_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { SSQ_F32 = 0, SSQ_F64 = 1 };
enum { SSQ_PAD_REFLECT = 0, SSQ_PAD_ZERO = 1 };          /* stft_utils.rs:19-65, utils/array.rs:52-98 */
/* upstream-variant plans and the *_host_v entry points only (utils/common.py:54-158): np.pad 'symmetric', 'edge', 'wrap'.
 * The reference-variant entry points keep their rule: 0 reflects, every other code pads with zeros. */
enum { SSQ_PAD_SYMMETRIC = 2, SSQ_PAD_REPLICATE = 3, SSQ_PAD_WRAP = 4 };
enum { SSQ_SQUEEZE_SUM = 0, SSQ_SQUEEZE_LEBESGUE = 1 };  /* ssq_stft.rs:292-296, ssq_cwt.rs:199-206 */
enum { SSQ_WAVELET_GMW = 0, SSQ_WAVELET_MORLET = 1 };    /* cwt.rs:496-543 */
enum { SSQ_FREQS_LOG = 0, SSQ_FREQS_LINEAR = 1 };        /* ssq_cwt.rs:56-112 */
/* upstream only (ssq_ssq_cwt_host_rows, _gmwk_rows): frequencies exponential on two segments (ssqueezing.py:247-283),
 * binned by algos.py:860-877 */
enum { SSQ_FREQS_LOG_PIECEWISE = 2 };
enum { SSQ_MAPRANGE_PEAK = 0, SSQ_MAPRANGE_MAXIMAL = 1 };/* ssq_cwt.rs:450-461 */
/* numerics variant of a plan / host call (bit flags).  0 = the Rust reference (rust/src/spectral/ *.rs).
 * SSQ_VARIANT_UPSTREAM = the vendored upstream ssqueezepy the Rust crate was derived from (SURVEY 8(f)-4,
 * /root/reference/old/ssqueezepy): pad split, Nyquist-zeroed diff-window, np.linspace frequencies, clamped
 * round-half-even bins, |.| > gamma, normalised wavelets with a halved Nyquist bin, p2up padding, ln2/nv constant.
 * MODULATED (STFT family, _stft.py:127-147) and FLIPUD (ssqueezing.py: k -> n-1-k) qualify UPSTREAM. */
enum { SSQ_VARIANT_RUST = 0, SSQ_VARIANT_UPSTREAM = 1, SSQ_VARIANT_MODULATED = 2, SSQ_VARIANT_FLIPUD = 4 };
/* what a STFT-family plan writes to its output */
enum {
  SSQ_OUT_TX  = 0,   /* synchrosqueezed STFT            (ssq_stft.rs:270-301) */
  SSQ_OUT_SX  = 1,   /* STFT                            (stft.rs:47-85)       */
  SSQ_OUT_DSX = 2,   /* derivative STFT                 (ssq_stft.rs:205-211,227) -- test hook */
  SSQ_OUT_WK  = 3    /* (w, k) per bin as (re, im)      (ssq_stft.rs:11-39,280-289) -- test hook */
};

/* ---- library / device ----------------------------------------------------- */
const char* ssq_last_error(void);
const char* ssq_hello_from_bin(void);                    /* lib.rs:16-19 */
int ssq_device_count(int* count);
int ssq_set_device(int device);
int ssq_device_info(int* cu_count, int64_t* hbm_bytes, char* name, int name_len);

/* ---- shape helpers (so callers can allocate outputs) ---------------------- */
/* stft.rs:32-34 / ssq_stft.rs:182-184 */
int ssq_stft_shape(int64_t n_signal, int64_t n_fft, int64_t hop, int64_t* n_freqs, int64_t* n_frames);
/* utils/array.rs:9-11 with cwt.rs:87,98: P = next_power_of_2(N + N/2), n1 = (P-N)/2 */
int ssq_cwt_pad_len(int64_t n_signal, int64_t* pad_len, int64_t* n1);
/* cwt.rs:461-489 / ssq_cwt.rs:300-326; simd_variant selects cwt_simd.rs:474-545.
 * Call with scales == NULL to obtain *na only. */
int ssq_log_scales(int64_t n_signal, int64_t nv, int simd_variant, int64_t* na, double* scales);
/* ssq_stft.rs:104-119: centre zero-pad / centre-crop `window[win_n]` to n_fft */
int ssq_size_window(const double* window, int64_t win_n, int64_t n_fft, double* out);
/* ssq_stft.rs:131-179: spectral derivative of the window (Nyquist term kept) */
int ssq_diff_window(const double* window, int64_t n_fft, double* out);
/* The index map every forward kernel fetches padded samples through: padded position m (m < 0 left of the signal,
 * m >= n right of it) -> *idx = source sample in [0, n), or -1 where the pad is zero.  Host code, no GPU needed.
 * Non-zero return for a pad type outside SSQ_PAD_* or n < 1. */
int ssq_pad_index(int padtype, int64_t m, int64_t n, int64_t* idx);
/* ssq_cwt.rs:450-469: the `ssq_freqs` vector ssq_cwt returns */
int ssq_cwt_ssq_freqs(const double* scales, int64_t na, int64_t n_signal, double dt,
                      int maprange, int freq_dist, double* ssq_freqs);

/* ---- host-pointer entry points (replace the PyO3 functions) ---------------- */
/* _rs.stft            rust/src/spectral/stft.rs:12-95
 * window has n_fft entries.  Sx: [batch][n_freqs][n_frames]; freqs: [n_freqs] (cycles/sample). */
int ssq_stft_host(int dtype, const void* x, int64_t batch, int64_t n_signal,
                  const double* window, int64_t n_fft, int64_t hop, int padtype,
                  void* Sx, double* freqs);

/* _rs.ssq_stft        rust/src/spectral/ssq_stft.rs:72-313
 * `window` is already sized to n_fft (ssq_size_window).  gamma < 0 selects the default
 * 10*EPS64 (ssq_stft.rs:258-261).  Tx: [batch][n_freqs][n_frames]; ssq_freqs: [n_freqs].
 * dbg_* may be NULL; when given they receive Sx, dSx (complex) and (w,k) pairs. */
int ssq_ssq_stft_host(int dtype, const void* x, int64_t batch, int64_t n_signal,
                      const double* window, int64_t n_fft, int64_t hop, double fs,
                      int padtype, int squeezing, double gamma,
                      void* Tx, double* ssq_freqs,
                      void* dbg_Sx, void* dbg_dSx, void* dbg_wk);

/* _rs.cwt / _rs.cwt_simd   rust/src/spectral/cwt.rs:46-144, cwt_simd.rs:52-150
 * Wx, dWx: [batch][na][cols], cols = rpadded ? P : N.  dWx may be NULL (derivative=False). */
int ssq_cwt_host(int dtype, const void* x, int64_t batch, int64_t n_signal,
                 int wavelet, const double* scales, int64_t na, double dt,
                 int l1_norm, int padtype, int rpadded,
                 void* Wx, void* dWx);

/* _rs.ssq_cwt         rust/src/spectral/ssq_cwt.rs:244-493
 * Tx: [batch][na][N]; ssq_freqs: [na] (not flipped).  dbg_* may be NULL:
 * Wx, dWx (unpadded, complex) and (w, k-or--1) pairs. */
int ssq_ssq_cwt_host(int dtype, const void* x, int64_t batch, int64_t n_signal,
                     int wavelet, const double* scales, int64_t na, double dt,
                     int freq_dist, int maprange, int padtype, int squeezing,
                     int flipud, double gamma,
                     void* Tx, double* ssq_freqs,
                     void* dbg_Wx, void* dbg_dWx, void* dbg_wk);

/* _rs.icwt            rust/src/spectral/cwt.rs:550-718   (implemented there, advertised by _rs.pyi:61-73, not registered)
 * Wx: [na][n_times] interleaved complex of `dtype`; scales: [n_scales_given >= na] (NULL -> "Scales must be
 * provided"); x_len < 0 selects n_times; x_out: [x_len] float64.  one_int: scaled row sum of Re Wx (:588-627);
 * otherwise the FFT filter bank of :629-714 for ANY x_len. */
int ssq_icwt_host(int dtype, const void* Wx, int64_t na, int64_t n_times, int wavelet, const double* scales,
                  int64_t n_scales_given, int one_int, int64_t x_len, double x_mean, int l1_norm, double* x_out);

/* wavelet helper functions (host side, fp64): rust/src/wavelets/morlet.rs:59-145, gmw.rs:236-357, _rs.pyi:89-132.
 * out: [n] interleaved complex128.  norm: "bandpass" (any case) or anything else = the L2 branch. */
int ssq_morlet(const double* w, int64_t n, double mu, double* out);
int ssq_morlet_freq(int64_t n, double scale, double mu, double* out);
int ssq_morlet_time(int64_t n, double scale, double mu, double* out);
int ssq_gmw(const double* w, int64_t n, double gamma, double beta, const char* norm, int order, double* out);
int ssq_gmw_freq(int64_t n, double scale, double gamma, double beta, const char* norm, int order, double* out);
int ssq_gmw_time(int64_t n, double scale, double gamma, double beta, const char* norm, int order, double* out);
int ssq_gmw_center_frequency(double gamma, double beta, const char* kind, double* out);

/* ---- upstream-parity mode and the inverses (/root/reference/old/ssqueezepy) ---------------------
 * ssqueezepy.stft      old/ssqueezepy/_stft.py:13-193  (window already n_fft long: get_window, :257-309, is host logic
 *                      of the Python mirror).  Sx, dSx: [batch][n_fft/2+1][(N-1)/hop+1]; dSx may be NULL. */
int ssq_stft_host_v(int dtype, const void* x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                    int64_t hop, double fs, int padtype, int variant, void* Sx, void* dSx);
/* ssqueezepy.ssq_stft  old/ssqueezepy/_ssq_stft.py:12-137 + algos.py:957-968.  gamma < 0: 10 eps of the dtype.
 * Sx, dSx, wk may be NULL; ssq_freqs: [n_freqs] (reversed with SSQ_VARIANT_FLIPUD). */
int ssq_ssq_stft_host_v(int dtype, const void* x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                        int64_t hop, double fs, int padtype, int squeezing, double gamma, int variant, void* Tx,
                        double* ssq_freqs, void* Sx, void* dSx, void* wk);
/* ssqueezepy.istft     old/ssqueezepy/_stft.py:196-254 (+ utils/stft_utils.py:141-191): per-frame inverse real FFT,
 * fftshift when modulated, windowed overlap-add, division by the window norm, unpadding.
 * Sx: [n_fft/2+1][n_frames] complex of `dtype`; window: [n_fft]; x_out: [N] real of `dtype`. */
int ssq_istft_host(int dtype, const void* Sx, int64_t n_frames, const double* window, int64_t n_fft, int64_t hop,
                   int64_t n_signal, int modulated, int win_exp, void* x_out);
/* The same for `batch` spectra Sx [batch][n_fft/2+1][n_frames] -> x_out [batch][N], one window and shape for all.
 * Power-of-two n_fft in 16 .. 4096 with hop <= n_fft and at least 256 tiles per signal (a tile: 16 frames, or twice the
 * (n_fft - 1) / hop frames that overlap a sample if that is more) run the streaming kernel of csrc/istft_fused.hip (one
 * pass over Sx, one write of x, no workspace beside them: tiles recompute the few frames they share); every other shape
 * runs the three-kernel path of ssq_istft_host one signal at a time.  The batch goes through the device in slices sized
 * from its free memory.  Signal b's result does not depend on `batch`.  SSQ_ISTFT_FUSED in the environment: 0 selects the
 * three-kernel path, 1 the streaming kernel wherever it takes the (n_fft, hop). */
int ssq_istft_batch_host(int dtype, const void* Sx, int64_t batch, int64_t n_frames, const double* window, int64_t n_fft,
                         int64_t hop, int64_t n_signal, int modulated, int win_exp, void* x_out);
/* The same on device buffers: d_Sx [batch][n_fft/2+1][n_frames], d_x [batch][N]; `window` on the host.  path -1: the
 * path ssq_istft_batch_host takes, 0: the three kernels per signal, 1: the fused kernel (an error where it does not take
 * the shape).  Synchronous.  kernel_ms (may be NULL): the time of the kernels alone, from HIP events around the launches
 * with tables and workspace set up before them. */
int ssq_istft_batch_exec(int dtype, const void* d_Sx, int64_t batch, int64_t n_frames, const double* window, int64_t n_fft,
                         int64_t hop, int64_t n_signal, int modulated, int win_exp, int path, void* d_x, float* kernel_ms);
/* Device bytes ssq_istft_batch_host needs beside one slice of Sx itself (x and the tables; for the three-kernel
 * path its per-signal [n_frames][n_fft] workspace), computed on the host; *fused (may be NULL) says which path the shape
 * takes.  -1 on a bad shape. */
int64_t ssq_istft_batch_workspace_bytes(int dtype, int64_t batch, int64_t n_frames, int64_t n_fft, int64_t hop,
                                        int64_t n_signal, int* fused);
/* Second-order ("vertical") synchrosqueezed STFT, `upstream.ssq_stft2` (csrc/stft_sst2.hip; upstream has no
 * such transform).  Conventions of ssq_ssq_stft_host_v: window [n_fft] already sized, padtype SSQ_PAD_*, squeezing
 * SSQ_SQUEEZE_*, gamma < 0: 10 eps of the dtype, variant: the SSQ_VARIANT_MODULATED and SSQ_VARIANT_FLIPUD bits (the
 * others are ignored).  n_fft must be a power of two from 16 to 4096.  Per-sample, with g1 = g', g2 = g'' (spectral
 * derivatives, Nyquist term zeroed), tg = u g, tg1 = u g1, u = j - n_fft/2, and V, V1, V2, Vt, Vt1 the STFTs with them:
 *   w1 = k/n_fft - (V1/V)/(2 pi i),  D = Vt V1 - Vt1 V,  q = (V2 V - V1^2)/(2 pi i D),  w2 = w1 - q Vt/V;
 *   the bin's frequency is fs |Re w2| where |D| > gamma^2 and Re w2 is finite, else fs |Re w1|; bins with |V| > gamma
 *   are reassigned by the upstream rule (clamped round-half-even on np.linspace(0, fs/2, n_freqs)), rows ascending.
 * Tx, Sx: [batch][n_freqs][n_frames] complex of `dtype`; ssq_freqs: [n_freqs] (reversed with FLIPUD; may be NULL);
 * w2 (may be NULL): [batch][n_freqs][n_frames] REAL of `dtype`, +inf where a bin is not kept.  Synchronous; the batch
 * goes through the device in slices sized from its free memory, and signal b's result does not depend on `batch`. */
int ssq_ssq_stft2_host(int dtype, const void* x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                       int64_t hop, double fs, int padtype, int squeezing, double gamma, int variant, void* Tx,
                       double* ssq_freqs, void* Sx, void* w2);
/* The fp64 window tables the transform is defined on, as the library builds them for `window` [n_fft] (host only, no
 * GPU): g1 = g', g2 = g'' (spectral derivatives, Nyquist term zeroed), tg = u g, tg1 = u g1, u = j - n_fft/2; each
 * [n_fft].  g2 is a second derivative by FFT: its rounding noise (1e-11 of its size at n_fft = 1024) differs between any
 * two FFTs that build it and moves the operator on ill-conditioned bins, so a reference takes the tables from here. */
int ssq_ssq_stft2_window_tables(const double* window, int64_t n_fft, double* g1, double* g2, double* tg, double* tg1);
/* Device bytes of the workspace ssq_ssq_stft2_exec needs (the packed map (w2, bin) of every bin and, for SSQ_F32, the
 * signals widened to fp64: the transforms and the operator run in fp64 for either dtype), computed on the host;
 * -1 on a shape ssq_ssq_stft2_host refuses. */
int64_t ssq_ssq_stft2_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t n_fft, int64_t hop);
/* The same transform on device buffers: d_x [batch][N], d_Tx, d_Sx, d_w2 (may be NULL) as above, d_workspace of at least
 * ssq_ssq_stft2_workspace_bytes bytes; `window` on the host.  Synchronous.  kernel_ms (may be NULL): the time of the
 * kernels alone (clearing Tx, the operator kernel, the scatter), from HIP events around the launches with the tables set
 * up before them. */
int ssq_ssq_stft2_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                       int64_t hop, double fs, int padtype, int squeezing, double gamma, int variant, void* d_Tx, void* d_Sx,
                       void* d_w2, void* d_workspace, int64_t workspace_bytes, float* kernel_ms);
/* Multisynchrosqueezed STFT, `upstream.mssq_stft` (csrc/stft_msst.hip; Yu, Wang and Zhao 2019; upstream has
 * no such transform): ssq_ssq_stft2_host whose frequency map is asked again at the bin a coefficient landed on, n_iter
 * steps in all.  Arguments, conventions and the n_fft range of ssq_ssq_stft2_host; order 1 or 2, n_iter 1 .. 64.  Per
 * column, with F = n_freqs and m[k] the one-step bin of row k -- ssq_ssq_stft2_host's bin rule on the frequency w the
 * call reports, BEFORE any flip, -1 where |V| <= gamma; order 2: that entry's w2 (with its fallback to w1), order 1:
 * fs |Re w1| on every bin (the same three transforms run for either order):
 *   c1[k] = m[k];   c(i+1)[k] = m[ci[k]] if ci[k] >= 0 and m[ci[k]] >= 0, else ci[k]        (i = 1 .. n_iter - 1)
 *   Tx[r(c_n[k])] += Sx[k] dw (SUM) or dw / F (LEBESGUE) for every kept k, rows ascending, in `dtype`, no atomics;
 *   r(b) = F - 1 - b with FLIPUD, else b.
 * A chain stops on a bin without a map of its own and on a fixed point; a cycle turns until n_iter runs out.  n_iter = 1,
 * order 2 is ssq_ssq_stft2_host bit for bit.  Tx, Sx, ssq_freqs as there; w (may be NULL): the ONE-step frequency map,
 * REAL of `dtype`, +inf where a bin is not kept; bins (may be NULL): [batch][n_freqs][n_frames] int32, the row of Tx each
 * coefficient went to (r applied), -1 where it was not kept.  Synchronous, sliced like ssq_ssq_stft2_host. */
int ssq_mssq_stft_host(int dtype, const void* x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                       int64_t hop, double fs, int padtype, int squeezing, double gamma, int variant, int order, int n_iter,
                       void* Tx, double* ssq_freqs, void* Sx, void* w, int32_t* bins);
/* Device bytes of the workspace ssq_mssq_stft_exec needs (ssq_ssq_stft2_workspace_bytes': the packed map and, for SSQ_F32,
 * the widened signals), computed on the host; -1 on a shape ssq_mssq_stft_host refuses. */
int64_t ssq_mssq_stft_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t n_fft, int64_t hop);
/* The same transform on device buffers: d_x [batch][N], d_Tx, d_Sx, d_w and d_bins (each may be NULL) as above,
 * d_workspace of at least ssq_mssq_stft_workspace_bytes bytes; `window` on the host.  Synchronous.  kernel_ms (may be
 * NULL): THREE floats, the time of the operator kernel (with the widening of a float32 call), of the walk kernel, and of
 * clearing Tx with the scatter, from HIP events around the launches with the tables set up before them. */
int ssq_mssq_stft_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                       int64_t hop, double fs, int padtype, int squeezing, double gamma, int variant, int order, int n_iter,
                       void* d_Tx, void* d_Sx, void* d_w, int32_t* d_bins, void* d_workspace, int64_t workspace_bytes,
                       float* kernel_ms);
/* The walk of ssq_mssq_stft_host alone, on maps the caller holds (the same kernel): bins_in, bins_out
 * [batch][n_rows][n_cols] int32 on the host, a target indexes the row axis itself, -1: no map.  n_rows 1 .. 2049,
 * n_iter 1 .. 64; a target outside -1 .. n_rows - 1 is refused on the host.  Synchronous. */
int ssq_msst_walk_host(const int32_t* bins_in, int64_t batch, int64_t n_rows, int64_t n_cols, int n_iter, int32_t* bins_out);
/* Columns of the tile one workgroup of the walk kernel holds in LDS for maps of n_rows rows (16 .. 256; host only), -1
 * outside 1 .. 2049. */
int ssq_msst_tile_cols(int64_t n_rows);
/* Time-reassigned synchrosqueezed STFT, `upstream.tssq_stft` (csrc/stft_tsst.hip; He, Tu, Bao, Hu and Zhang
 * 2019; upstream has no such transform): every coefficient moves along TIME to its estimated group delay.  window [n_fft]
 * already sized, padtype SSQ_PAD_*, order 1 or 2, gamma < 0: 10 eps of the dtype (NaN is refused), variant: the
 * SSQ_VARIANT_MODULATED bit (the others are ignored).  n_fft must be a power of two from 16 to 4096.  Per-sample, with
 * the window tables and the STFTs V, V1, V2, Vt, Vt1 of ssq_ssq_stft2_host, frame m centred on sample m hop:
 *   d1 = Re(Vt/V),  D = Vt V1 - Vt1 V,  num = V2 V - V1^2,  d2 = Re(Vt/V + V1 D / (V num));
 *   offset = d2 where order = 2, |num| > gamma^2, d2 is finite and |d2| <= n_fft/2, else d1; clamped to +- n_fft/2;
 *   tau = offset / fs in `dtype`, +inf where |V| <= gamma;  r = rint(tau / (hop/fs)) in `dtype` (0 where not finite);
 *   m' = clip(m + r, 0, n_frames - 1);  Tx[k][m'] += Sx[k][m] exp(-2 pi i ((k (m - m') hop) mod n_fft) / n_fft), every
 *   cell in ascending source frame (no atomics: signal b's result does not depend on `batch` or on the tiling).
 * Tx, Sx: [batch][n_freqs][n_frames] complex of `dtype`; tau (may be NULL): [batch][n_freqs][n_frames] REAL of `dtype`,
 * seconds relative to the frame's own time.  Synchronous; the batch goes through the device in slices sized from its
 * free memory. */
int ssq_tssq_stft_host(int dtype, const void* x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                       int64_t hop, double fs, int padtype, int order, double gamma, int variant, void* Tx, void* Sx,
                       void* tau);
/* Device bytes of the workspace ssq_tssq_stft_exec needs (for SSQ_F32 the signals widened to fp64, then one int16
 * relative target per bin), computed on the host; -1 on a shape ssq_tssq_stft_host refuses. */
int64_t ssq_tssq_stft_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t n_fft, int64_t hop);
/* The same transform on device buffers: d_x [batch][N], d_Tx, d_Sx, d_tau (may be NULL) as above, d_workspace of at least
 * ssq_tssq_stft_workspace_bytes bytes; `window` on the host.  Synchronous.  kernel_ms (may be NULL): TWO floats, the
 * time of the operator kernel (with the widening of a float32 call) and of the time scatter, from HIP events around
 * the launches with the tables set up before them. */
int ssq_tssq_stft_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                       int64_t hop, double fs, int padtype, int order, double gamma, int variant, void* d_Tx, void* d_Sx,
                       void* d_tau, void* d_workspace, int64_t workspace_bytes, float* kernel_ms);
/* Time-reassigned multisynchrosqueezed STFT, `upstream.tmssq_stft` (csrc/stft_tmsst.hip; Yu, Lin, Ma and He
 * 2020; upstream has no such transform): ssq_tssq_stft_host whose time map is asked again at the frame a coefficient
 * landed on, n_iter steps in all.  Arguments, conventions and the n_fft range of ssq_tssq_stft_host; order 1 or 2, n_iter
 * 1 .. 64, and n_iter H <= 16384 with H = ceil(n_fft / (2 hop)) (the final relative target is an int16 and a tile of
 * targets with both halos is staged in LDS).  Per row, with t[m] = m' of ssq_tssq_stft_host for a kept bin, none where
 * |V| <= gamma:
 *   c1[m] = t[m];   c(i+1)[m] = t[ci[m]] if t[ci[m]] is kept, else ci[m]                  (i = 1 .. n_iter - 1)
 *   Tx[k][c_n[m]] += Sx[k][m] exp(-2 pi i ((k (m - c_n[m]) hop) mod n_fft) / n_fft) for every kept m, every cell in
 *   ascending source frame (a compensated fp64 sum, no atomics: the result does not depend on `batch` or on the tiling).
 * A chain stops on a frame whose bin of that row is not kept and on a fixed point; a cycle turns until n_iter runs out.
 * n_iter = 1 is ssq_tssq_stft_host bit for bit.  Tx, Sx as there; tau (may be NULL): the ONE-step map, REAL of `dtype`,
 * +inf where a bin is not kept; targets (may be NULL): [batch][n_freqs][n_frames] int32, the frame of Tx each
 * coefficient went to, -1 where it was not kept.  Synchronous, sliced like ssq_tssq_stft_host. */
int ssq_tmssq_stft_host(int dtype, const void* x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                        int64_t hop, double fs, int padtype, int order, double gamma, int variant, int n_iter, void* Tx,
                        void* Sx, void* tau, int32_t* targets);
/* Device bytes of the workspace ssq_tmssq_stft_exec needs (ssq_tssq_stft_workspace_bytes' and one more int16 per bin,
 * the walked targets), computed on the host; -1 on a shape ssq_tmssq_stft_host refuses (n_iter enters through
 * n_iter H <= 16384). */
int64_t ssq_tmssq_stft_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t n_fft, int64_t hop, int n_iter);
/* The same transform on device buffers: d_x [batch][N], d_Tx, d_Sx, d_tau and d_targets (each may be NULL) as above,
 * d_workspace of at least ssq_tmssq_stft_workspace_bytes bytes; `window` on the host.  Synchronous.  kernel_ms (may be
 * NULL): THREE floats, the time of the operator kernel (with the widening of a float32 call), of the walk kernel (0 work
 * at n_iter = 1 without d_targets: no launch), and of the time scatter, from HIP events around the launches with the
 * tables set up before them. */
int ssq_tmssq_stft_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                        int64_t hop, double fs, int padtype, int order, double gamma, int variant, int n_iter, void* d_Tx,
                        void* d_Sx, void* d_tau, int32_t* d_targets, void* d_workspace, int64_t workspace_bytes,
                        float* kernel_ms);
/* The walk of ssq_tmssq_stft_host alone, on maps the caller holds (the same kernel): targets_in, targets_out
 * [batch][n_rows][n_frames] int32 on the host, a target indexes the frame axis itself, -1: none.  n_iter 1 .. 64,
 * reach >= 1, n_iter reach <= 16384; a target outside -1 .. n_frames - 1 or farther than `reach` from its own frame is
 * refused on the host.  Synchronous. */
int ssq_tmsst_walk_host(const int32_t* targets_in, int64_t batch, int64_t n_rows, int64_t n_frames, int n_iter, int64_t reach,
                        int32_t* targets_out);
/* Target frames of the tile one workgroup of the walk kernel (and of the scatter) owns for one-step targets within `reach`
 * frames walked n_iter steps (1024 .. 4096; host only), -1 where ssq_tmsst_walk_host refuses the pair. */
int ssq_tmsst_tile_frames(int64_t reach, int n_iter);
/* Synchroextracting and transient-extracting STFT, `upstream.set_stft` (axis 0; Yu, Yu and Zhang 2017; second order: Bao
 * et al. 2019) and `upstream.tet_stft` (axis 1; Yu 2019) (csrc/stft_extract.hip; upstream has no such
 * transform): a coefficient is KEPT where its own estimate says it already sits on the ridge, and zeroed elsewhere;
 * nothing moves.  window [n_fft] already sized, padtype SSQ_PAD_*, axis 0 (frequency) or 1 (time), order 1 or 2,
 * gamma < 0: 10 eps of the dtype (NaN is refused), variant: the SSQ_VARIANT_MODULATED bit (the others are ignored).  n_fft
 * must be a power of two from 16 to 4096.  In fp64 for either dtype, with F = n_fft/2 + 1 and a cell LIVE where
 * |V| > gamma:
 *   axis 0: w = the frequency ssq_ssq_stft2_host reports: fs |Re w2| where order = 2, |D| > gamma^2 and Re w2 is finite,
 *           else fs |Re w1| (order 1: on every cell, from the ONE transform x (g + i g1)); rounded once to `dtype`, +inf
 *           where the cell is not live;  b = the clamped round-half-even bin of w on np.linspace(0, fs/2, F), taken in
 *           `dtype` (ssq_ssq_stft2_host's rule, no flipud);  the cell is kept where b == k;
 *   axis 1: tau = the offset ssq_tssq_stft_host reports, in seconds and `dtype`: d2 with its fallback to d1, clamped to
 *           +- n_fft/2 (order 1: d1, from the ONE transform x (g + i tg)), +inf where the cell is not live;
 *           r = rint(tau / (hop/fs)) in `dtype`, BEFORE ssq_tssq_stft_host's clip to the frame range (an edge cell that
 *           the clip would bring back onto itself is not kept);  the cell is kept where r == 0;
 *   Te[k][m] = Sx[k][m] where the cell is live and kept, else +0 + 0i.  The rows of Te are the rows of Sx.
 * Te holds exactly the coefficients that ssq_mssq_stft_host(order, n_iter = 1) leaves on their own row (axis 0) and that
 * ssq_tssq_stft_host would move by r = 0 (axis 1).  Every cell is written exactly once by ONE kernel; signal b's bits do
 * not depend on `batch`, the slice or the workspace.  Te: [batch][n_freqs][n_frames] complex of `dtype`; Sx (may be
 * NULL): the same shape, equal to the STFT; map (may be NULL): [batch][n_freqs][n_frames] REAL of `dtype`, w (axis 0) or
 * tau (axis 1).  There is no inverse.  Synchronous; the batch goes through the device in slices sized from its free
 * memory. */
int ssq_extract_stft_host(int dtype, const void* x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                          int64_t hop, double fs, int padtype, int axis, int order, double gamma, int variant, void* Te,
                          void* Sx, void* map);
/* Device bytes of the workspace ssq_extract_stft_exec needs: for SSQ_F32 the signals widened to fp64 (8 batch n_signal),
 * for SSQ_F64 none (0); computed on the host; -1 on a shape ssq_extract_stft_host refuses. */
int64_t ssq_extract_stft_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t n_fft, int64_t hop);
/* The same transform on device buffers: d_x [batch][N], d_Te, d_Sx (may be NULL), d_map (may be NULL) as above,
 * d_workspace of at least ssq_extract_stft_workspace_bytes bytes (where that is 0, d_workspace may be NULL); `window` on
 * the host.  Synchronous.  kernel_ms (may be NULL): ONE float, the time of the kernel (with the widening of a float32
 * call), from HIP events around the launches with the tables set up before them. */
int ssq_extract_stft_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                          int64_t hop, double fs, int padtype, int axis, int order, double gamma, int variant, void* d_Te,
                          void* d_Sx, void* d_map, void* d_workspace, int64_t workspace_bytes, float* kernel_ms);
/* Reassigned spectrogram, `upstream.reassign_stft` (csrc/stft_reassign.hip; Kodera et al. 1978; Auger and
 * Flandrin 1995; upstream has no such transform): every bin's energy |Sx|^2 moves along frequency AND time at once, to
 * its instantaneous frequency and its group delay (first order only).  window [n_fft] already sized, padtype SSQ_PAD_*,
 * gamma < 0: 10 eps of the dtype (NaN is refused), variant: the SSQ_VARIANT_MODULATED bit (the others are ignored).
 * n_fft must be a power of two from 16 to 4096.  Per-sample, with the window tables g, g1, tg and the STFTs V, V1, Vt of
 * ssq_ssq_stft2_host, frame m centred on sample m hop, in fp64 for either dtype:
 *   w = fs |k/n_fft - Im(V1/V)/(2 pi)|,  tau = clamp(Re(Vt/V), +- n_fft/2) / fs, each rounded once to `dtype`, +inf where
 *   |V| <= gamma;  k' = ssq_ssq_stft2_host's bin rule on w (np.linspace(0, fs/2, n_freqs), no flip);
 *   m' = clip(m + rint(tau / (hop/fs)), 0, n_frames - 1) in `dtype`;  Rx[k'][m'] += |Sx[k][m]|^2 (of the reported Sx, in
 *   fp64), accumulated in 64-bit fixed point with the quantum P 2^-38, P the smallest power of two >= the signal's
 *   max |Sx|^2: integer adds commute, so signal b's result does not depend on `batch`, the tiling or the order.
 * Rx: [batch][n_freqs][n_frames] REAL of `dtype`; Sx: the same shape, complex of `dtype`; w, tau (each may be NULL):
 * REAL of `dtype`, Hz and seconds relative to the frame's own time.  Synchronous; the batch goes through the device in
 * slices sized from its free memory. */
int ssq_reassign_stft_host(int dtype, const void* x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                           int64_t hop, double fs, int padtype, double gamma, int variant, void* Rx, void* Sx, void* w,
                           void* tau);
/* Device bytes of the workspace ssq_reassign_stft_exec needs (for SSQ_F32 the signals widened to fp64, then 8 bytes a
 * signal for its max |Sx|^2 and one packed 4-byte target per bin), computed on the host; -1 on a shape
 * ssq_reassign_stft_host refuses. */
int64_t ssq_reassign_stft_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t n_fft, int64_t hop);
/* The same transform on device buffers: d_x [batch][N], d_Rx, d_Sx, d_w and d_tau (each may be NULL) as above,
 * d_workspace of at least ssq_reassign_stft_workspace_bytes bytes; `window` on the host.  Synchronous.  kernel_ms (may be
 * NULL): TWO floats, the time of the operator kernel (with the widening of a float32 call) and of the scatter, from HIP
 * events around the launches with the tables set up before them. */
int ssq_reassign_stft_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                           int64_t hop, double fs, int padtype, double gamma, int variant, void* d_Rx, void* d_Sx,
                           void* d_w, void* d_tau, void* d_workspace, int64_t workspace_bytes, float* kernel_ms);
/* ssqueezepy.issq_stft / issq_cwt, full inverse (_ssq_stft.py:139-198, _ssq_cwt.py:313-378):
 * x_out[j] = scale * sum_rows row_scale[row] * Re Tx[row][j]   (scale = 2 / window[n_fft/2]  resp.  2 / adm_ssq;
 * row_scale NULL = 1; the one-integral icwt of _cwt.py:477-492 is the same sum with 1/sqrt(a) rows for the L2 norm).
 * Tx: [rows][cols] complex of `dtype`; x_out: [cols] real of `dtype`. */
int ssq_issq_host(int dtype, const void* Tx, int64_t rows, int64_t cols, double scale, const double* row_scale,
                  void* x_out);
/* The same for Tx [batch][rows][cols] -> x_out [batch][cols]; entry b equals ssq_issq_host on Tx[b] bit for bit.
 * row_scale [rows] (shared by the batch) may be NULL. */
int ssq_issq_batch_host(int dtype, const void* Tx, int64_t batch, int64_t rows, int64_t cols, double scale,
                        const double* row_scale, void* x_out);
/* upstream wavelets: SSQ_WAVELET_GMW with (p0, p1) = (gamma, beta), L1 / bandpass norm (_gmw.py:187-210);
 * SSQ_WAVELET_MORLET with p0 = mu (wavelets.py:497-523).
 * adm_ssq = int_0^inf conj(psih(w)) / w dw, adm_cwt = int |psih|^2 / w (utils/cwt_utils.py:28-63, trapezoid on the
 * grids of integrate_analytic, :583-627); the peak centre frequency on the padded grid (wavelets.py:713-716). */
int ssq_upstream_adm(int wavelet, double p0, double p1, int which_cwt, double* out);
int ssq_upstream_center_frequency(int wavelet, double p0, double p1, double scale, int64_t n_padded, double* wc);
/* utils/common.py:32-51: padded length 2^(1 + round(log2 n)), left pad n1 >= right pad n2 */
int ssq_upstream_p2up(int64_t n_signal, int64_t* n_up, int64_t* n1, int64_t* n2);
/* wavelet.fn of the upstream wavelet at scale 1 (wavelets.py:409-523; GMW bandpass order 0: p0 = gamma, p1 = beta;
 * Morlet: p0 = mu), fp64, for the scale search of utils/cwt_utils.py: out[i] = psih(w[i]), i < n.  Host only. */
int ssq_upstream_psih(int wavelet, double p0, double p1, const double* w, int64_t n, double* out);
/* ssqueezepy.cwt       old/ssqueezepy/_cwt.py:12-318 with explicit scales.  Wx, dWx: [batch][na][cols],
 * cols = rpadded ? n_up : N; dWx may be NULL. */
int ssq_cwt_host_v(int dtype, const void* x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                   const double* scales, int64_t na, double dt, int l1_norm, int padtype, int rpadded, int variant,
                   void* Wx, void* dWx);
/* ssqueezepy.ssq_cwt   old/ssqueezepy/_ssq_cwt.py:12-311 + ssqueezing.py:122-146 + algos.py:899-910 (exponential
 * scales, difftype 'trig').  ssq_freqs_asc: [na] the ascending frequencies the bins refer to (the caller reverses
 * them like ssqueezing.py:199-205); nv: voices per octave of `scales` (the constant ln2/nv).
 * Wx, dWx, wk may be NULL. */
int ssq_ssq_cwt_host_v(int dtype, const void* x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                       const double* scales, int64_t na, double dt, int nv, const double* ssq_freqs_asc, int freq_dist,
                       int padtype, int squeezing, double gamma, int variant, void* Tx, void* Wx, void* dWx, void* wk);
/* Higher-order upstream GMW(gamma, beta), bandpass norm (_gmw.py:267-295, :366-395; _cwt.py:515-608):
 *   psih(w) = C(w) exp(-beta ln wc + wc^gamma + beta ln w - w^gamma) for w > 0, C(w) = sum_m coeffs[m] (2 w^gamma)^m,
 * Nyquist bin halved.  Order k is coeffs = k_consts of _gmw_k_constants (order 0: {2}); an averaged order set is ONE
 * polynomial, the mean of the orders' k_consts padded with zeros (the transform is linear in the wavelet).
 * coeffs: [n_groups][n_coeffs], 1 <= n_coeffs <= 17 (orders up to 16), finite; variant must include
 * SSQ_VARIANT_UPSTREAM.  cwt: Wx, dWx [batch][n_groups][na][cols] -- group g is the transform with polynomial g, all
 * groups from one forward FFT per signal; na * n_groups <= 32767.  ssq_cwt: n_groups must be 1; ssq_freqs_asc comes
 * from the caller (upstream: the order-0 wavelet's). */
int ssq_cwt_host_gmwk(int dtype, const void* x, int64_t batch, int64_t n_signal, double gamma, double beta,
                      const double* coeffs, int64_t n_coeffs, int64_t n_groups, const double* scales, int64_t na,
                      double dt, int l1_norm, int padtype, int rpadded, int variant, void* Wx, void* dWx);
int ssq_ssq_cwt_host_gmwk(int dtype, const void* x, int64_t batch, int64_t n_signal, double gmw_gamma, double gmw_beta,
                          const double* coeffs, int64_t n_coeffs, int64_t n_groups, const double* scales, int64_t na,
                          double dt, int nv, const double* ssq_freqs_asc, int freq_dist, int padtype, int squeezing,
                          double gamma, int variant, void* Tx, void* Wx, void* dWx, void* wk);
/* ssq_ssq_cwt_host_v / _gmwk on any upstream scale grid (ssqueezing.py:122-133, algos.py:860-897); the two above are
 * these with row_const[i] = ln2/nv.  variant must include SSQ_VARIANT_UPSTREAM.
 *   row_const: [na] finite, the weight of row i, out[k, j] += Wx[i, j] * row_const[i] (squeezing 'lebesgue':
 *              row_const[i] / na): ln2 / nv[i] for 'log' / 'log-piecewise' scales (nv per row: nv_from_scales),
 *              (s[1] - s[0]) / s[i] for 'linear' scales;
 *   freq_kind: SSQ_FREQS_LOG, SSQ_FREQS_LINEAR or SSQ_FREQS_LOG_PIECEWISE -- the bin rule of ssq_freqs_asc;
 *   freq_transition: SSQ_FREQS_LOG_PIECEWISE only (ignored otherwise): the index idx, 2 <= idx <= na-1, splitting
 *              ssq_freqs_asc into [:idx] and [idx:] (logscale_transition_idx, cwt_utils.py:375-395, found by the caller
 *              on the frequencies in their own dtype); the second segment's bins start at row idx-1 (algos.py:364-370). */
int ssq_ssq_cwt_host_rows(int dtype, const void* x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                          const double* scales, int64_t na, double dt, const double* row_const,
                          const double* ssq_freqs_asc, int freq_kind, int64_t freq_transition, int padtype,
                          int squeezing, double gamma, int variant, void* Tx, void* Wx, void* dWx, void* wk);
int ssq_ssq_cwt_host_gmwk_rows(int dtype, const void* x, int64_t batch, int64_t n_signal, double gmw_gamma,
                               double gmw_beta, const double* coeffs, int64_t n_coeffs, int64_t n_groups,
                               const double* scales, int64_t na, double dt, const double* row_const,
                               const double* ssq_freqs_asc, int freq_kind, int64_t freq_transition, int padtype,
                               int squeezing, double gamma, int variant, void* Tx, void* Wx, void* dWx, void* wk);
/* Second-order ("vertical") synchrosqueezed CWT, `upstream.ssq_cwt2` (csrc/cwt_sst2.hip; upstream has no
 * such transform).  Arguments as ssq_ssq_cwt_host_rows (wavelet SSQ_WAVELET_GMW with (gamma, beta) or _MORLET with mu;
 * variant: the SSQ_VARIANT_FLIPUD bit, the others are ignored; gamma < 0: 10 eps of the dtype).  Per-sample, with
 * P = p2up(n_signal), xh the DFT of the padded signal, xi_k = 2 pi k / P for k <= P/2 (zero tables above), and for
 * scale a the fp64 tables T0 = psih(a xi), T1 = a psih'(a xi) (both halved at 2k == P):
 *   W = F^-1[xh T0], W1 = F^-1[xh i xi T0], W2 = F^-1[xh (-xi^2) T0], Wt = F^-1[xh (-i) T1], Wt1 = F^-1[xh xi T1];
 *   D = W^2 + Wt1 W - Wt W1,  c = (W2 W - W1^2) / D,  om1 = W1 / W,  om2 = om1 - c Wt / W;
 *   w2 = |Im om2| / (2 pi dt) where |D| > gamma^2 and Im om2 is finite, else |Im om1| / (2 pi dt); +inf where |W| < gamma.
 * Wx = W (upstream's L1-normalised cwt); Tx = the scatter of Wx under w2 by ssq_ssqueeze_w_exec's rule.  Transforms and
 * operator run in fp64 for either dtype; Wx and w2 are rounded once on store and the scatter runs on the rounded values.
 * Tx, Wx: [batch][na][n_signal] complex of `dtype`; w2: the same shape, REAL of `dtype` (host: may be NULL).
 * The batch x na rows go through the workspace in chunks of R rows: 16 P (batch + 10 R) bytes; a row's result does not
 * depend on R or on the batch.  work_limit_bytes: 0 for the preferred size, else at least min_bytes. */
int ssq_ssq_cwt2_host(int dtype, const void* x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                      const double* scales, int64_t na, double dt, const double* row_const, const double* ssq_freqs_asc,
                      int freq_kind, int64_t freq_transition, int padtype, int squeezing, double gamma, int variant,
                      int64_t work_limit_bytes, void* Tx, void* Wx, void* w2);
/* Device bytes of the workspace: returns the preferred size (every row in one chunk, capped at 2 GiB) and stores the
 * least one (one row per chunk) in *min_bytes (may be NULL); computed on the host; -1 on a bad shape. */
int64_t ssq_ssq_cwt2_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t na, int64_t* min_bytes);
/* The same transform on device buffers: d_x [batch][n_signal], d_Tx, d_Wx, d_w2 (required) as above, d_workspace of
 * workspace_bytes >= min_bytes (its size sets R); scales, row_const, ssq_freqs_asc on the host.  Synchronous on
 * `stream`.  kernel_ms (may be NULL): the time of the kernels alone, from HIP events around the launches. */
int ssq_ssq_cwt2_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                      const double* scales, int64_t na, double dt, const double* row_const, const double* ssq_freqs_asc,
                      int freq_kind, int64_t freq_transition, int padtype, int squeezing, double gamma, int variant,
                      void* d_Tx, void* d_Wx, void* d_w2, void* d_workspace, int64_t workspace_bytes, void* stream,
                      float* kernel_ms);
/* The two fp64 tables of one scale on the host (no GPU), by the functions the kernel evaluates them with
 * (csrc/cwt_sst2_wavelets.h): T0, T1 [P], zero above P/2.  P a power of two. */
int ssq_ssq_cwt2_tables(int wavelet, double p0, double p1, double scale, int64_t P, double* T0, double* T1);
/* Multisynchrosqueezed CWT, `upstream.mssq_cwt` (csrc/cwt_msst.hip; the CWT counterpart of
 * ssq_mssq_stft_host; upstream has no such transform): ssq_ssq_cwt2_host whose frequency map is asked again at the row
 * nearest to the bin a coefficient landed on, n_iter steps in all.  Arguments and conventions of ssq_ssq_cwt2_host; order
 * 1 or 2, n_iter 1 .. 64, na 2 .. 2049.  Per column, with w[i] the one-step frequency of row i in `dtype` (order 2: that
 * entry's w2 with its fallback; order 1: |Im om1| / (2 pi dt) on every element; +inf where |W| < gamma), b[i] the bin of
 * w[i] by ssq_ssqueeze_w_exec's rule BEFORE any flip (-1 where w is infinite; NaN: bin 0) and row_of_bin [na] (host,
 * every entry in 0 .. na - 1; `upstream.mssq_cwt_row_of_bin` builds the row nearest to each bin in log frequency):
 *   r1[k] = k (kept k);   r(i+1)[k] = row_of_bin[b[ri[k]]] if b[row_of_bin[b[ri[k]]]] >= 0, else ri[k]   (i = 1 .. n_iter - 1)
 *   w_n[k] = w[r_n[k]], +inf where k is not kept;   Tx = the scatter of Wx under w_n by ssq_ssqueeze_w_exec (FLIPUD there).
 * A chain stops on a row without a map of its own and on a fixed point; a cycle turns until n_iter runs out.  n_iter = 1,
 * order 2 is ssq_ssq_cwt2_host bit for bit.  Tx, Wx as there; w (may be NULL): the ONE-step frequency, REAL of `dtype`;
 * rows (may be NULL): [batch][na][n_signal] int32, r_n, -1 where not kept; bins (may be NULL): int32, b.  Synchronous. */
int ssq_mssq_cwt_host(int dtype, const void* x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                      const double* scales, int64_t na, double dt, const double* row_const, const double* ssq_freqs_asc,
                      int freq_kind, int64_t freq_transition, int padtype, int squeezing, double gamma, int variant,
                      int64_t work_limit_bytes, int order, int n_iter, const int32_t* row_of_bin, void* Tx, void* Wx, void* w,
                      int32_t* rows, int32_t* bins);
/* Device bytes of the workspace ssq_mssq_cwt_exec needs: the plane of w_n ([batch][na][n_signal] REAL of `dtype`, to a
 * multiple of 16 bytes) in front of ssq_ssq_cwt2_workspace_bytes' workspace.  Returns the preferred size and stores the
 * least one in *min_bytes (may be NULL); computed on the host; -1 on a shape ssq_mssq_cwt_host refuses. */
int64_t ssq_mssq_cwt_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t na, int64_t* min_bytes);
/* The same transform on device buffers: d_x [batch][n_signal], d_Tx, d_Wx, d_w (required), d_rows and d_bins (each may be
 * NULL) as above, d_workspace of workspace_bytes >= min_bytes; scales, row_const, ssq_freqs_asc, row_of_bin on the host.
 * n_iter = 1 with neither d_rows nor d_bins launches no walk kernel.  Synchronous on `stream`.  kernel_ms (may be NULL):
 * THREE floats, the time of the pipeline with the operator, of the walk kernel, and of clearing Tx with the scatter, from
 * HIP events around the launches with the tables set up before them. */
int ssq_mssq_cwt_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                      const double* scales, int64_t na, double dt, const double* row_const, const double* ssq_freqs_asc,
                      int freq_kind, int64_t freq_transition, int padtype, int squeezing, double gamma, int variant, int order,
                      int n_iter, const int32_t* row_of_bin, void* d_Tx, void* d_Wx, void* d_w, int32_t* d_rows,
                      int32_t* d_bins, void* d_workspace, int64_t workspace_bytes, void* stream, float* kernel_ms);
/* The walk of ssq_mssq_cwt_host alone, on frequency maps the caller holds (the same kernel): w, w_n [batch][na][n_cols]
 * REAL of `dtype` and rows, bins int32 of the same shape, all on the host and all required; +inf in w: not kept.  na
 * 2 .. 2049, n_cols 1 .. 2^30, n_iter 1 .. 64; a row_of_bin entry outside 0 .. na - 1 is refused on the host.
 * Synchronous. */
int ssq_mssq_cwt_walk_host(int dtype, const void* w, int64_t batch, int64_t na, int64_t n_cols, const double* ssq_freqs_asc,
                           int freq_kind, int64_t freq_transition, const int32_t* row_of_bin, int n_iter, int32_t* rows,
                           int32_t* bins, void* w_n);
/* Columns of the tile one workgroup of the walk kernel holds in LDS for `na` rows (16 .. 256; host only), -1 outside
 * 2 .. 2049. */
int ssq_mssq_cwt_tile_cols(int64_t na);
/* Reassigned scalogram, `upstream.reassign_cwt` (csrc/cwt_reassign.hip; Auger and Flandrin 1995, III;
 * upstream has no such transform): every coefficient's energy |Wx|^2 moves along frequency AND time at once, to its
 * instantaneous frequency and its group delay (first order only).  Arguments as ssq_ssq_cwt2_host without row weights
 * and squeezing (variant: the SSQ_VARIANT_FLIPUD bit; gamma < 0: 10 eps of the dtype, NaN is refused).  Per-sample, with
 * P, xh, xi_k, T0, T1 of ssq_ssq_cwt2_host, in fp64 for either dtype:
 *   W = F^-1[xh T0], W1 = F^-1[xh i xi T0], Wt = F^-1[xh (-i) T1];
 *   w = |Im(W1/W)| / (2 pi dt),  tau = clamp(Re(Wt/W), +- n_signal) dt, each rounded once to `dtype`, +inf where
 *   |W| < gamma;  k' = ssq_ssqueeze_w_exec's bin rule on the reported w in `dtype` (flipped with the variant bit);
 *   m' = clip(j + rint(tau / dt), 0, n_signal - 1) in `dtype`;  Rx[k'][m'] += |Wx[i][j]|^2 (of the reported Wx, in fp64),
 *   accumulated by 64-bit integer atomic adds in fixed point with the quantum Pmax 2^-S, S = min(38, 62 -
 *   ceil(log2(na n_signal))), Pmax the smallest power of two >= the signal's max |Wx|^2: integer adds commute, so signal
 *   b's result depends neither on `batch`, nor on the chunking, nor on the order.  na * n_signal <= 2^40.
 * Rx: [batch][na][n_signal] REAL of `dtype`; Wx: the same shape, complex of `dtype` (ssq_ssq_cwt2_host's Wx); w, tau
 * (each may be NULL): REAL of `dtype`, Hz and seconds relative to the column's own time; kk, mm (each may be NULL): int32,
 * the targets k' and m', -1 where a bin is not kept.
 * Workspace: 16 ceil(batch / 2) + 16 batch na n_signal bytes (the maxima, the accumulators, the targets), then
 * 16 P (batch + 6 R) for chunks of R rows; a row's result does not depend on R or on the batch.  work_limit_bytes: 0 for
 * the preferred size, else at least min_bytes. */
int ssq_reassign_cwt_host(int dtype, const void* x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                          const double* scales, int64_t na, double dt, const double* ssq_freqs_asc, int freq_kind,
                          int64_t freq_transition, int padtype, double gamma, int variant, int64_t work_limit_bytes,
                          void* Rx, void* Wx, void* w, void* tau, void* kk, void* mm);
/* Device bytes of the workspace: returns the preferred size (every row in one chunk, the chunk area capped at 2 GiB) and
 * stores the least one (one row per chunk) in *min_bytes (may be NULL); computed on the host; -1 on a bad shape. */
int64_t ssq_reassign_cwt_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t na, int64_t* min_bytes);
/* The same transform on device buffers: d_x [batch][n_signal], d_Rx, d_Wx (required), d_w, d_tau, d_kk, d_mm (each may be
 * NULL) as above, d_workspace of workspace_bytes >= min_bytes (its size sets R); scales, ssq_freqs_asc on the host.
 * Synchronous on `stream`.  kernel_ms (may be NULL): TWO floats, the time of all the kernels and of the scatter kernel
 * alone, from HIP events around the launches. */
int ssq_reassign_cwt_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                          const double* scales, int64_t na, double dt, const double* ssq_freqs_asc, int freq_kind,
                          int64_t freq_transition, int padtype, double gamma, int variant, void* d_Rx, void* d_Wx,
                          void* d_w, void* d_tau, void* d_kk, void* d_mm, void* d_workspace, int64_t workspace_bytes,
                          void* stream, float* kernel_ms);
/* Time-reassigned synchrosqueezed CWT, `upstream.tssq_cwt` (csrc/cwt_tsst.hip; upstream has no such
 * transform): every complex coefficient moves along TIME inside its own row, to its group delay, rotated so that its
 * phase refers to the target column.  scales, wavelet, p0, p1, dt, padtype, gamma as ssq_ssq_cwt2_host (gamma < 0: 10 eps
 * of the dtype, NaN is refused); row_freqs [na]: nu_i = wc / (2 pi scales[i]) cycles/sample in fp64, positive and finite,
 * the caller's (`upstream.tssq_cwt_row_freqs`); order 1 or 2.  Per-sample, with P, xh, xi_k, T0, T1 and the five maps
 * W, W1, W2, Wt, Wt1 of ssq_ssq_cwt2_host (order 1 forms W and Wt alone), in fp64 for either dtype:
 *   d1 = Re(Wt/W);  D = W^2 + Wt1 W - Wt W1;  num = W2 W - W1^2;  d2 = d1 - Im((D/num) (2 pi nu_i + i W1/W));
 *   off = d2 where order = 2, |num| > gamma^2, d2 is finite and |d2| <= n_signal, else d1; clamped to +- n_signal;
 *   tau = off dt rounded once to `dtype`, +inf where |W| < gamma;  m' = clip(j + rint(tau / dt), 0, n_signal - 1) in
 *   `dtype`;  Tx[i][m'] += Wx[i][j] exp(-2 pi i frac(nu_i (j - m'))) (of the reported Wx, in fp64), accumulated by two
 *   64-bit integer atomic adds in fixed point with the quantum A 2^-S, S = min(38, 61 - ceil(log2 n_signal)), A the
 *   smallest power of two >= sqrt(Pmax), Pmax the smallest power of two >= the signal's max |Wx|^2: integer adds
 *   commute, so signal b's result depends neither on `batch`, nor on the chunking, nor on the order.
 *   na * n_signal <= 2^40.
 * Tx, Wx: [batch][na][n_signal] complex of `dtype` (Wx: ssq_ssq_cwt2_host's); tau (may be NULL): REAL of `dtype`, seconds
 * relative to the column's own time; mm (may be NULL): int32, the target m', -1 where a bin is not kept.
 * Workspace: 16 ceil(batch / 2) + 20 batch na n_signal bytes (to a multiple of 16: the maxima, the accumulators, the
 * targets), then 16 P (batch + 2 M R) for chunks of R rows, M = 2 (order 1) or 5 (order 2); a row's result does not
 * depend on R or on the batch.  work_limit_bytes: 0 for the preferred size, else at least min_bytes. */
int ssq_tssq_cwt_host(int dtype, const void* x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                      const double* scales, const double* row_freqs, int64_t na, double dt, int padtype, int order,
                      double gamma, int64_t work_limit_bytes, void* Tx, void* Wx, void* tau, void* mm);
/* Device bytes of the workspace: returns the preferred size (every row in one chunk, the chunk area capped at 2 GiB) and
 * stores the least one (one row per chunk) in *min_bytes (may be NULL); computed on the host; -1 on a bad shape. */
int64_t ssq_tssq_cwt_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t na, int order, int64_t* min_bytes);
/* The same transform on device buffers: d_x [batch][n_signal], d_Tx, d_Wx (required), d_tau, d_mm (each may be NULL) as
 * above, d_workspace of workspace_bytes >= min_bytes (its size sets R); scales, row_freqs on the host.  Synchronous on
 * `stream`.  kernel_ms (may be NULL): THREE floats, the time of all the kernels, of the scatter kernel alone and of
 * everything before the scatter, from HIP events around the launches. */
int ssq_tssq_cwt_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                      const double* scales, const double* row_freqs, int64_t na, double dt, int padtype, int order,
                      double gamma, void* d_Tx, void* d_Wx, void* d_tau, void* d_mm, void* d_workspace,
                      int64_t workspace_bytes, void* stream, float* kernel_ms);
/* Time-reassigned multisynchrosqueezed CWT, `upstream.tmssq_cwt` (csrc/cwt_tmsst.hip; the iteration of Yu,
 * Lin, Ma and He 2020 on ssq_tssq_cwt_host's time map; upstream has no such transform): the map is asked again at the
 * column a coefficient landed on, n_iter steps in all.  Arguments, conventions and limits of ssq_tssq_cwt_host; order 1
 * or 2, n_iter 1 .. 64.  Per row, with t[j] = m' of ssq_tssq_cwt_host for a kept bin, none where |W| < gamma:
 *   c1[j] = t[j];   c(k+1)[j] = t[ck[j]] if t[ck[j]] is kept, else ck[j]                  (k = 1 .. n_iter - 1)
 *   Tx[i][c_n[j]] += Wx[i][j] exp(-2 pi i frac(nu_i (j - c_n[j]))) for every kept j, accumulated as there (the same
 *   quantum: a cell still takes at most n_signal contributions), so Tx is bitwise independent of the order of the adds,
 *   of the chunking and of `batch`.
 * A chain stops on a column that is not kept and on a fixed point; a cycle turns until n_iter runs out.  A target may lie
 * anywhere in its row (the offset is clamped to +- n_signal, not to a window), so the walk reads the steps that leave
 * its staged tile from device memory.  n_iter = 1 is ssq_tssq_cwt_host bit for bit (no walk is launched).  Tx, Wx as
 * there; tau (may be NULL): the ONE-step map; mm (may be NULL): int32, the column of Tx each coefficient went to, -1
 * where it was not kept.  Workspace: ssq_tssq_cwt_host's with 24 bytes a cell in the head where that has 20 (the walked
 * plane).  The walk runs after all chunks. */
int ssq_tmssq_cwt_host(int dtype, const void* x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                       const double* scales, const double* row_freqs, int64_t na, double dt, int padtype, int order,
                       double gamma, int n_iter, int64_t work_limit_bytes, void* Tx, void* Wx, void* tau, void* mm);
/* Device bytes of the workspace, as ssq_tssq_cwt_workspace_bytes reports them: the preferred size returned, the least
 * one in *min_bytes (may be NULL); computed on the host; -1 on a bad shape. */
int64_t ssq_tmssq_cwt_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t na, int order, int64_t* min_bytes);
/* The same transform on device buffers, as ssq_tssq_cwt_exec.  Synchronous on `stream`.  kernel_ms (may be NULL): FOUR
 * floats, the time of all the kernels, of the operator part (everything before the walk), of the walk kernel (no launch
 * at n_iter = 1) and of the scatter kernel, from HIP events around the launches. */
int ssq_tmssq_cwt_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                       const double* scales, const double* row_freqs, int64_t na, double dt, int padtype, int order,
                       double gamma, int n_iter, void* d_Tx, void* d_Wx, void* d_tau, void* d_mm, void* d_workspace,
                       int64_t workspace_bytes, void* stream, float* kernel_ms);
/* The walk of ssq_tmssq_cwt_host alone, on maps the caller holds (the same kernel, launched at n_iter = 1 too):
 * targets_in, targets_out [batch][n_rows][n_cols] int32 on the host, a target indexes the column axis itself, -1: none.
 * n_cols 1 .. 2^30, n_iter 1 .. 64; a target outside -1 .. n_cols - 1 is refused on the host.  Synchronous, the batch
 * sliced to the device's free memory. */
int ssq_tmssq_cwt_walk_host(const int32_t* targets_in, int64_t batch, int64_t n_rows, int64_t n_cols, int n_iter,
                            int32_t* targets_out);
/* Columns of the tile one workgroup of the walk kernel owns; *halo (may be NULL): the columns it stages on either side of
 * the tile.  Host only. */
int ssq_tmssq_cwt_tile_cols(int* halo);
/* Synchroextracting and transient-extracting CWT, `upstream.set_cwt` (axis 0) and `upstream.tet_cwt` (axis 1)
 * (csrc/cwt_extract.hip; the CWT counterpart of ssq_extract_stft_host; upstream has neither): a coefficient
 * is KEPT where its own estimate says it sits on the ridge and zeroed elsewhere.  Arguments, conventions and limits of
 * ssq_tssq_cwt_host without its na * n_signal limit (there is no accumulator); axis 0 or 1, order 1 or 2.  With the maps
 * of ssq_ssq_cwt2_host in fp64 for either dtype, a cell live unless |W| < gamma:
 *   axis 0: w = ssq_ssq_cwt2_host's w2 (order 2, with its fallback) or |Im(W1/W)| / (2 pi dt) on every cell (order 1, from
 *           W and W1 alone), rounded once to `dtype`, +inf where the cell is not live;  row_edges [na + 1], Hz, fp64, the
 *           caller's (`upstream.set_cwt_row_edges`): e[0] = +inf, e[na] = 0, never increasing, no NaN; each is rounded
 *           once to `dtype`;  keep where e[i+1] <= w < e[i], compared in `dtype` (a NaN w is kept nowhere).
 *   axis 1: tau = ssq_tssq_cwt_host's reported offset (order 2: d2 with its fallback to d1; order 1: d1, from W and Wt
 *           alone), +inf where the cell is not live;  keep where rint(tau / dt) == 0 in `dtype`, the relative target
 *           BEFORE that entry's clip to the signal.
 *   Te[i][j] = Wx[i][j] where the cell is live and kept, else +0 + 0i.
 * row_freqs [na] (ssq_tssq_cwt_host's) is required for axis 1 and row_edges for axis 0; the one the axis does not use may
 * be NULL (it is checked if given).  Te (required), Wx (may be NULL): [batch][na][n_signal] complex of `dtype`, Wx
 * ssq_ssq_cwt2_host's; map (may be NULL): REAL of `dtype`, w in Hz or tau in seconds.  One operator kernel writes every
 * cell exactly once.  Workspace: 16 P (batch + 2 M R) bytes for chunks of R rows and nothing else, M = 2 (order 1) or 5
 * (order 2); a row's result does not depend on R or on the batch.  work_limit_bytes: 0 for the preferred size, else at
 * least min_bytes. */
int ssq_extract_cwt_host(int dtype, const void* x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                         const double* scales, const double* row_freqs, const double* row_edges, int64_t na, double dt,
                         int padtype, int axis, int order, double gamma, int64_t work_limit_bytes, void* Te, void* Wx,
                         void* map);
/* Device bytes of the workspace: returns the preferred size (every row in one chunk, capped at 2 GiB) and stores the
 * least one (one row per chunk) in *min_bytes (may be NULL); computed on the host; -1 on a bad shape. */
int64_t ssq_extract_cwt_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t na, int order, int64_t* min_bytes);
/* The same transform on device buffers: d_x [batch][n_signal], d_Te (required), d_Wx, d_map (each may be NULL) as above,
 * d_workspace of workspace_bytes >= min_bytes (its size sets R; one byte less is refused before any launch); scales,
 * row_freqs, row_edges on the host.  Synchronous on `stream`.  kernel_ms (may be NULL): ONE float, the time of the kernels
 * alone, from HIP events around the launches. */
int ssq_extract_cwt_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                         const double* scales, const double* row_freqs, const double* row_edges, int64_t na, double dt,
                         int padtype, int axis, int order, double gamma, void* d_Te, void* d_Wx, void* d_map,
                         void* d_workspace, int64_t workspace_bytes, void* stream, float* kernel_ms);
/* Local maximum synchrosqueezed STFT, `upstream.lmssq_stft` (csrc/stft_lmsst.hip; Yu, Wang, Zhao and Liu
 * 2019; upstream has no such transform).  Arguments as ssq_mssq_stft_host (n_fft a power of two from 16 to 4096, squeezing
 * SUM or LEBESGUE, the MODULATED and FLIPUD bits of `variant`, gamma < 0: 10 eps of the dtype), with `delta` from 1 to
 * min(n_fft / 2, 256) in place of order and n_iter.  No derivative of the window is formed: ONE fp64 transform x g per
 * frame.  Per column, F = n_fft / 2 + 1 rows:
 *   A[k] = re^2 + im^2 of Sx[k] as reported (rounded to `dtype`), in fp64, the products and the sum rounded one by one;
 *   m[k] = the row of the maximum of A over max(0, k - delta) .. min(F - 1, k + delta), scanned ascending and taken only
 *          where strictly greater (the lowest row wins a tie; rows that are not kept take part);
 *   Tx[r(m[k])] += Sx[k] dw (SUM) or dw / F (LEBESGUE) for the kept k (|V| > gamma in fp64), rows ascending, in `dtype`,
 *          no atomics;  r(b) = F - 1 - b under FLIPUD, else b.
 * ONE kernel decides a column in LDS and writes every cell of Tx exactly once: nothing is cleared and there is no map in
 * device memory.  Tx, Sx (both required): [batch][n_freqs][n_frames] complex of `dtype`; ssq_freqs (may be NULL):
 * [n_freqs] fp64; bins (may be NULL): int32, the row of Tx a coefficient went to, -1 where it was not kept.
 * Synchronous; the batch goes through the device in slices sized from its free memory. */
int ssq_lmssq_stft_host(int dtype, const void* x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                        int64_t hop, double fs, int padtype, int squeezing, double gamma, int variant, int delta, void* Tx,
                        double* ssq_freqs, void* Sx, int32_t* bins);
/* Device bytes of the workspace ssq_lmssq_stft_exec needs: for SSQ_F32 the signals widened to fp64 (8 batch n_signal),
 * for SSQ_F64 none (0); computed on the host; -1 on a shape ssq_lmssq_stft_host refuses. */
int64_t ssq_lmssq_stft_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t n_fft, int64_t hop);
/* The same transform on device buffers: d_x [batch][n_signal], d_Tx, d_Sx (required), d_bins (may be NULL) as above,
 * d_workspace of at least ssq_lmssq_stft_workspace_bytes (NULL with 0 bytes for SSQ_F64); window on the host.
 * Synchronous.  kernel_ms (may be NULL): ONE float, the time of the kernels alone, from HIP events around the launches. */
int ssq_lmssq_stft_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                        int64_t hop, double fs, int padtype, int squeezing, double gamma, int variant, int delta, void* d_Tx,
                        void* d_Sx, int32_t* d_bins, void* d_workspace, int64_t workspace_bytes, float* kernel_ms);
/* Local maximum synchrosqueezed CWT, `upstream.lmssq_cwt` (csrc/cwt_lmsst.hip; the CWT counterpart of
 * ssq_lmssq_stft_host).  Arguments as ssq_ssq_cwt2_host, for 2 .. 2049 scales, with `delta` from 1 to min(na - 1, 256) and
 * row_freqs_hz [na], the rows' own frequencies in Hz (positive, finite; `upstream.tssq_cwt_row_freqs` / dt), each rounded
 * once to `dtype`.  A map set of W alone: ONE inverse transform a row.  Per column, with A and m as above over the na
 * rows of Wx as reported: w[i] = row_freqs_hz[m[i]], +inf where |W| < gamma on the fp64 coefficient; rows[i] = m[i], -1
 * there; Tx = ssqueeze(Wx, w) by ssq_ssqueeze_w_exec, so a coefficient keeps its own row weight and phase.  Tx, Wx
 * (required), w (REAL of `dtype`), rows (int32) (each may be NULL): [batch][na][n_signal]; Wx is ssq_ssq_cwt2_host's bit
 * for bit.  Workspace: 16 P (batch + 2 R) bytes for chunks of R rows; a row's result depends neither on R nor on the
 * batch.  work_limit_bytes: 0 for the preferred size, else at least min_bytes. */
int ssq_lmssq_cwt_host(int dtype, const void* x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                       const double* scales, int64_t na, double dt, const double* row_const, const double* ssq_freqs_asc,
                       int freq_kind, int64_t freq_transition, int padtype, int squeezing, double gamma, int variant,
                       int64_t work_limit_bytes, int delta, const double* row_freqs_hz, void* Tx, void* Wx, void* w,
                       int32_t* rows);
/* Device bytes of the workspace: returns the preferred size (every row in one chunk, capped at 2 GiB) and stores the
 * least one (one row per chunk) in *min_bytes (may be NULL); computed on the host; -1 on a bad shape. */
int64_t ssq_lmssq_cwt_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t na, int64_t* min_bytes);
/* The same transform on device buffers: d_Tx, d_Wx, d_w (required), d_rows (may be NULL) as above, d_workspace of
 * workspace_bytes >= min_bytes; the tables on the host.  Synchronous on `stream`.  kernel_ms (may be NULL): THREE floats,
 * the time of the transforms with the Wx kernel, of the plane kernel (the window maximum), and of the squeeze. */
int ssq_lmssq_cwt_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                       const double* scales, int64_t na, double dt, const double* row_const, const double* ssq_freqs_asc,
                       int freq_kind, int64_t freq_transition, int padtype, int squeezing, double gamma, int variant, int delta,
                       const double* row_freqs_hz, void* d_Tx, void* d_Wx, void* d_w, int32_t* d_rows, void* d_workspace,
                       int64_t workspace_bytes, void* stream, float* kernel_ms);
/* The plane kernel of ssq_lmssq_cwt_host alone, `upstream.lmsst_rows`: A [batch][n_rows][n_cols] REAL of `dtype` on the
 * host (a float32 map is widened on load, which is exact), rows [same shape] int32: m as above, with no keep rule.
 * n_rows 2 .. 2049, n_cols 1 .. 2^30, delta 1 .. min(n_rows - 1, 256).  Synchronous, the batch sliced to the device's
 * free memory. */
int ssq_lmsst_rows_host(int dtype, const void* A, int64_t batch, int64_t n_rows, int64_t n_cols, int delta, int32_t* rows);
/* ConceFT, the multitaper synchrosqueezed CWT, `upstream.conceft_cwt` (csrc/cwt_conceft.hip; Daubechies,
 * Wang and Wu 2016; upstream has no such transform).  The wavelets are the GMWs (gmw_gamma, gmw_beta; bandpass norm) of
 * n_orders distinct orders, coeffs [n_orders][n_coeffs] their polynomials as for ssq_cwt_host_gmwk (1 <= n_orders <= 8,
 * na * n_orders <= 32767); vectors [n_draws][n_orders] complex (interleaved, fp64), the caller's unit vectors already
 * gauged (`upstream.conceft_vectors`), 1 <= n_draws <= 256; scale: C_0 / sum_m c_m > 0 (`upstream.gmw_adm_ssq`).  scales,
 * dt, row_const, ssq_freqs_asc, freq_kind, freq_transition, padtype as ssq_ssq_cwt_host_rows; gamma < 0: 10 eps of the
 * dtype, NaN is refused; variant: the SSQ_VARIANT_FLIPUD bit.  With W_g, dW_g the planes of ssq_cwt_host_gmwk (l1_norm,
 * not rpadded), in `dtype`:
 *   W^(m) = sum_g vectors[m][g] W_g, dW^(m) likewise (g ascending);  k = the bin of ssq_ssq_cwt_host_rows' rule on
 *   (W^(m), dW^(m)), kept where |W^(m)| > gamma;  Tx[k][n] += W^(m)[i][n] * (row_const[i] * scale rounded to `dtype`).
 * One thread owns a column: no atomics, the additions into a cell in a fixed order (draws in chunks of 8; chunks, then
 * rows, then draws ascending; a draw's run of rows in one bin is summed first), so a signal's result depends neither on
 * `batch` nor on the workspace.  Squeezing 'sum' only.
 * Tx: [batch][na][n_signal] complex of `dtype`; Wx (may be NULL): [batch][n_orders][na][n_signal] complex, the planes W_g;
 * w (may be NULL): [batch][n_draws][na][n_signal] REAL of `dtype`, every draw's phase transform, +inf where not kept.
 * Workspace: 32 (fp32: 16) n_orders na n_signal bytes per signal of a slice (to a multiple of 256).  work_limit_bytes:
 * 0 for the preferred size, else at least min_bytes.  Beside that workspace the call holds on the device only as many
 * signals (x, Tx and the Wx and w asked for) as fit, in slices of the batch (at most ssq_host_slice_cap signals). */
int ssq_conceft_cwt_host(int dtype, const void* x, int64_t batch, int64_t n_signal, double gmw_gamma, double gmw_beta,
                         const double* coeffs, int64_t n_coeffs, int64_t n_orders, const double* vectors, int64_t n_draws,
                         double scale, const double* scales, int64_t na, double dt, const double* row_const,
                         const double* ssq_freqs_asc, int freq_kind, int64_t freq_transition, int padtype, double gamma,
                         int variant, int64_t work_limit_bytes, void* Tx, void* Wx, void* w);
/* Device bytes of the workspace: returns the preferred size (the whole batch in one slice, capped at 1 GiB but never
 * below one signal) and stores the least one (one signal per slice) in *min_bytes (may be NULL); computed on the host;
 * -1 on a bad shape. */
int64_t ssq_conceft_cwt_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t na, int64_t n_orders,
                                        int64_t* min_bytes);
/* The same transform on device buffers: d_x [batch][n_signal], d_Tx (required), d_Wx, d_w (each may be NULL) as above,
 * d_workspace of workspace_bytes >= min_bytes (its size sets the signals per slice); coeffs, vectors, scales, row_const,
 * ssq_freqs_asc on the host.  Synchronous on `stream`.  kernel_ms (may be NULL): ONE float, the time of the squeeze
 * kernel alone (summed over the slices), from HIP events around its launches. */
int ssq_conceft_cwt_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, double gmw_gamma, double gmw_beta,
                         const double* coeffs, int64_t n_coeffs, int64_t n_orders, const double* vectors, int64_t n_draws,
                         double scale, const double* scales, int64_t na, double dt, const double* row_const,
                         const double* ssq_freqs_asc, int freq_kind, int64_t freq_transition, int padtype, double gamma,
                         int variant, void* d_Tx, void* d_Wx, void* d_w, void* d_workspace, int64_t workspace_bytes,
                         void* stream, float* kernel_ms);
/* ConceFT on the STFT, the multitaper synchrosqueezed STFT, `upstream.conceft_stft` (csrc/stft_conceft.hip, DESIGN 4.19;
 * Daubechies, Wang and Wu 2016; upstream has no such transform).  tapers [n_tapers][n_fft]: real windows already sized
 * to n_fft (1 <= n_tapers <= 8; n_fft a power of two from 16 to 4096); vectors [n_draws][n_tapers] complex (interleaved,
 * fp64), the caller's unit vectors already gauged so that c_m = sum_j vectors[m][j] tapers[j][n_fft/2] > 0,
 * 1 <= n_draws <= 256; scale: tapers[0][n_fft/2] / sum_m c_m > 0.  hop, fs, padtype as ssq_ssq_stft2_host; gamma < 0:
 * 10 eps of the dtype, NaN is refused; variant: the SSQ_VARIANT_MODULATED and SSQ_VARIANT_FLIPUD bits.  With V_j, V1_j
 * the STFTs of x with tapers[j] and its spectral derivative (Nyquist term zeroed), computed in fp64 and rounded once to
 * `dtype`, then in `dtype`:
 *   S = sum_j vectors[m][j] V_j, dS likewise from V1_j (j ascending);  w = fs |k/n_fft - Im(dS/S)/(2 pi)|, kept where
 *   |S| > gamma;  b = ssq_ssq_stft2_host's bin of w on linspace(0, fs/2, F);  Tx[b][t] += S * (dw * scale rounded to
 *   `dtype`), dw = the grid's step.
 * One thread owns a column: no atomics, the additions into a cell in a fixed order (draws in chunks of 8; chunks, then
 * rows, then draws ascending; a draw's run of rows in one bin is summed first), so a signal's result depends neither on
 * `batch` nor on the workspace.
 * Tx: [batch][F][n_frames] complex of `dtype`, F = n_fft/2 + 1, n_frames = (n_signal - 1)/hop + 1; ssq_freqs (may be
 * NULL): F doubles; Sx, dSx (each may be NULL): [batch][n_tapers][F][n_frames] complex, the planes V_j, V1_j; w (may be
 * NULL): [batch][n_draws][F][n_frames] REAL of `dtype`, every draw's frequency, +inf where not kept.
 * Workspace: the 2 n_tapers planes of a slice, 32 (fp32: 16) n_tapers F bytes per frame, plus 8 n_signal bytes per
 * signal of a slice for a float32 call; a slice is whole signals, or a run of whole store tiles (4096 / n_fft frames)
 * of one signal.  work_limit_bytes: 0 for the preferred size, else at least min_bytes.  Beside that workspace the call
 * holds on the device only as many signals (x, Tx and the Sx, dSx and w asked for) as fit, in slices of the batch (at most
 * ssq_host_slice_cap signals). */
int ssq_conceft_stft_host(int dtype, const void* x, int64_t batch, int64_t n_signal, const double* tapers, int64_t n_tapers,
                          int64_t n_fft, int64_t hop, double fs, int padtype, const double* vectors, int64_t n_draws,
                          double scale, double gamma, int variant, int64_t work_limit_bytes, void* Tx, double* ssq_freqs,
                          void* Sx, void* dSx, void* w);
/* Device bytes of the workspace: returns the preferred size (whole signals up to 1 GiB; never below the least; the squeeze
 * kernel runs one wave per 64 frames of a slice, so a larger workspace is faster until a slice holds some 200 000 frames)
 * and stores the least one (one store tile of one signal) in *min_bytes (may be NULL); computed on the host; -1 on a bad
 * shape. */
int64_t ssq_conceft_stft_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t n_fft, int64_t hop,
                                         int64_t n_tapers, int64_t* min_bytes);
/* The same transform on device buffers: d_x [batch][n_signal], d_Tx (required), d_Sx, d_dSx, d_w (each may be NULL) as
 * above, d_workspace of workspace_bytes >= min_bytes (its size sets the slices); tapers, vectors on the host.
 * Synchronous on `stream`.  kernel_ms (may be NULL): TWO floats, the time of the squeeze kernel alone and of the plane
 * kernel alone (each summed over the slices), from HIP events around their launches. */
int ssq_conceft_stft_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, const double* tapers,
                          int64_t n_tapers, int64_t n_fft, int64_t hop, double fs, int padtype, const double* vectors,
                          int64_t n_draws, double scale, double gamma, int variant, void* d_Tx, void* d_Sx, void* d_dSx,
                          void* d_w, void* d_workspace, int64_t workspace_bytes, void* stream, float* kernel_ms);

/* ---- plans: device-resident batch pipelines -------------------------------- */
typedef struct ssq_stft_plan ssq_stft_plan;
/* One plan = one (dtype, N, n_fft, hop, window, fs, padtype, squeezing, gamma) configuration.
 * force_generic != 0 selects the unfused any-n_fft kernels (test hook). */
int ssq_stft_plan_create(ssq_stft_plan** plan, int dtype, int64_t n_signal,
                         const double* window, int64_t n_fft, int64_t hop, double fs,
                         int padtype, int squeezing, double gamma, int force_generic);
/* the same with a numerics variant (SSQ_VARIANT_*); upstream plans run on the unfused kernels */
int ssq_stft_plan_create_v(ssq_stft_plan** plan, int dtype, int64_t n_signal,
                           const double* window, int64_t n_fft, int64_t hop, double fs,
                           int padtype, int squeezing, double gamma, int force_generic, int variant);
int ssq_stft_plan_destroy(ssq_stft_plan* plan);
/* 1 if the fused LDS-tile kernel serves this plan, 0 if the generic kernels do */
int ssq_stft_plan_is_fused(const ssq_stft_plan* plan);
/* bytes of device scratch exec needs for `batch` signals with output kind `out_kind` */
int64_t ssq_stft_plan_workspace_bytes(const ssq_stft_plan* plan, int64_t batch, int out_kind);
/* Read-only: what ssq_stft_plan_exec would launch for `out_kind` and `batch` signals on the fused kernels --
 * frames per output tile, tiles over the whole batch and the grid (persistent blocks: each walks
 * ceil(total_tiles / max_blocks) tiles at most).  Where a pass is an interior launch plus an edge launch, total_tiles
 * is their sum and max_blocks the larger grid.  Plans on the unfused kernels report tile_frames = 0 (and 0 tiles).
 * Out-pointers may be NULL.  Launches nothing. */
int ssq_stft_plan_launch_info(const ssq_stft_plan* plan, int out_kind, int64_t batch, int* tile_frames,
                              int64_t* total_tiles, int64_t* max_blocks);
/* The same per launch, in launch order: n_launch is 0 (unfused plan), 1 or 2; for launch i, edge[i] is 1 for the
 * edge-capable kernel (padding by index mirroring) and 0 for the interior kernel (direct loads), tiles[i] its tiles
 * over the batch, blocks[i] its grid.  The arrays hold at least 2 entries; any pointer may be NULL. */
int ssq_stft_plan_launch_list(const ssq_stft_plan* plan, int out_kind, int64_t batch, int* n_launch, int* edge,
                              int64_t* tiles, int64_t* blocks);
/* Read-only: the kernel family ssq_stft_plan_exec launches for `out_kind`, read from the fields the launcher itself
 * branches on.  DFT: direct sums (dft_frames_kernel); FFT_BATCHED: frames packed for the batched any-length device FFT;
 * FUSED_POW2 / FUSED_SPLIT: stft_fused_kernel on a power of two (SPLIT: the fp64 n_fft = 1024 configuration);
 * TX1024: stft_tx1024_kernel (fp32 n_fft = 1024, Tx and (w, k)); MIXED_RADIX / BLUESTEIN: the any-length modes of
 * stft_fused_kernel.  Launches nothing. */
enum {
  SSQ_STFT_ROUTE_DFT = 0,
  SSQ_STFT_ROUTE_FFT_BATCHED = 1,
  SSQ_STFT_ROUTE_FUSED_POW2 = 2,
  SSQ_STFT_ROUTE_FUSED_SPLIT = 3,
  SSQ_STFT_ROUTE_TX1024 = 4,
  SSQ_STFT_ROUTE_MIXED_RADIX = 5,
  SSQ_STFT_ROUTE_BLUESTEIN = 6
};
int ssq_stft_plan_route(const ssq_stft_plan* plan, int out_kind, int* route);
/* d_x: [batch][N]; d_out: [batch][n_freqs][n_frames] complex; async on `stream` (hipStream_t). */
int ssq_stft_plan_exec(ssq_stft_plan* plan, int out_kind, const void* d_x, int64_t batch,
                       void* d_out, void* d_workspace, int64_t workspace_bytes, void* stream);

/* The same over a STRIDED batch of n_groups * group signals: signal s starts at
 * d_x + (s / group) * group_stride + (s % group) * sig_stride (elements); windows may overlap.
 * This is how the chunked-overlap front end (tests/stft_ssq_test.py:216-281: map_overlap with depth = n_fft) runs
 * all extended chunks of all channels as one batch: group = chunks per channel, sig_stride = chunk,
 * group_stride = channel pitch.  d_out: [n_groups * group][n_freqs][n_frames]. */
int ssq_stft_plan_exec_strided(ssq_stft_plan* plan, int out_kind, const void* d_x, int64_t n_groups,
                               int64_t group, int64_t group_stride, int64_t sig_stride, void* d_out,
                               void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- chunked-overlap multi-channel front end (device side) ------------------
 * Replaces the Dask harness around `_rs.*`: tests/stft_ssq_test.py:163-283, tests/ssq_cwt_test.py:66-195. */
/* d_xext: [channels][depth + samples + depth]; the middle already holds the channel.  Fills the two array-end
 * halos like dask.map_overlap(boundary="reflect") (mirror INCLUDING the edge sample; boundary = 1: zeros). */
int ssq_chunk_halo_fill(int dtype, void* d_xext, int64_t channels, int64_t samples, int64_t depth,
                        int boundary, void* stream);
/* (channels, chunks, rows, cols) -> (rows, all chunks' columns, channels), the reference's np.transpose(stacked,
 * (1, 2, 0)) plus the concatenation of the chunk outputs (stft_ssq_test.py:265-267), complex elements of `dtype`:
 * out[(r*out_cols + out_col_base + j*ncols + c)*out_channels + ch_base + ch] = in[((ch*chunks + j)*rows + r)*cols_in + col0 + c] */
int ssq_chunks_relayout(int dtype, const void* d_in, int64_t channels, int64_t chunks, int64_t rows,
                        int64_t cols_in, int64_t col0, int64_t ncols, void* d_out, int64_t out_cols,
                        int64_t out_col_base, int64_t out_channels, int64_t ch_base, void* stream);

typedef struct ssq_cwt_plan ssq_cwt_plan;
/* na <= 32767 (with a higher-order GMW: na * n_groups <= 32767): the scale rows sit on grid.y of the table kernels, and a
 * plan with more is refused at creation ("too many scales (max 32767)"), as are the *_host calls that build one. */
int ssq_cwt_plan_create(ssq_cwt_plan** plan, int dtype, int64_t n_signal, int wavelet,
                        const double* scales, int64_t na, double dt, int padtype);
/* the same with a numerics variant (SSQ_VARIANT_*) and the upstream wavelet's parameters (p0, p1) = (gamma, beta) of
 * the GMW or (mu, -) of the Morlet wavelet; upstream plans pad by p2up and run on the generic transforms */
int ssq_cwt_plan_create_v(ssq_cwt_plan** plan, int dtype, int64_t n_signal, int wavelet, double p0, double p1,
                          const double* scales, int64_t na, double dt, int padtype, int variant);
/* the higher-order upstream GMW (coeffs, n_coeffs, n_groups as for ssq_cwt_host_gmwk): the plan has na * n_groups rows,
 * row g * na + i = scales[i] with polynomial g; exec_ssq needs n_groups == 1 */
int ssq_cwt_plan_create_gmwk(ssq_cwt_plan** plan, int dtype, int64_t n_signal, double gamma, double beta,
                             const double* coeffs, int64_t n_coeffs, int64_t n_groups, const double* scales, int64_t na,
                             double dt, int padtype, int variant);
int ssq_cwt_plan_destroy(ssq_cwt_plan* plan);
int64_t ssq_cwt_plan_workspace_bytes(const ssq_cwt_plan* plan, int64_t batch);
/* How many scales of an ssq exec the cwt_os families serve (time tiles, decimated, analytic-input and full-circle
 * tiles).  0: the naive / tile / two-step / big kernels alone, which is what every upstream-variant plan gets. */
int ssq_cwt_plan_tiled_rows(const ssq_cwt_plan* plan);
/* Which scales each cwt_os family of an fp32 ssq exec serves, as half-open row ranges read from the fields the launcher
 * itself uses: out = {os_a0, os_s0, os_mid, os_s1, os_d1, os_z0, os_z1, reg}.  [os_a0, os_s0): analytic-input tiles,
 * [os_s0, os_mid): 4096-point tiles, [os_mid, os_s1): 8192-point tiles, [os_s1, os_d1): 16-fold decimated tiles,
 * [os_z0, os_z1): full-circle phase blocks; reg: the other two-step scales run on the register core.  Rows in front of
 * the first tiled one are reassigned before the tiles (plain stores into the cleared Tx), rows behind it after them
 * (read-modify-write).  An empty range: that family is not launched. */
int ssq_cwt_plan_tile_segments(const ssq_cwt_plan* plan, int32_t out[8]);
/* cwt: d_Wx/d_dWx [batch][na][cols]; d_dWx may be NULL */
int ssq_cwt_plan_exec_cwt(ssq_cwt_plan* plan, const void* d_x, int64_t batch, int l1_norm,
                          int rpadded, void* d_Wx, void* d_dWx,
                          void* d_workspace, int64_t workspace_bytes, void* stream);
/* ssq_cwt: d_Tx [batch][na][N]; d_dbg_* may be NULL */
int ssq_cwt_plan_exec_ssq(ssq_cwt_plan* plan, const void* d_x, int64_t batch,
                          int freq_dist, int maprange, int squeezing, int flipud, double gamma,
                          void* d_Tx, void* d_dbg_Wx, void* d_dbg_dWx, void* d_dbg_wk,
                          void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- ridge extraction: ssqueezepy.extract_ridges (old/ssqueezepy/ridge_extraction.py:11-233) -------------------
 * Tf: [batch][n_freqs][n_time], complex (interleaved) when is_complex, in `dtype` (the energy / cost / DP type, :121).
 * param_dtype: the dtype of scales, eps and penalty (:113-116) -- SSQ_F64 only for complex128 upstream, so
 * (SSQ_F64, SSQ_F32) is the fp64-cost / fp32-parameter case of real float64 input; (SSQ_F32, SSQ_F64) is rejected.
 * metric: [n_freqs] in param_dtype, log(scales) for 'cwt' else scales (:118-120), from which the kernels form
 * P[i, j] = penalty * (m_i - m_j)**2 (:89).  scales: [n_freqs] in param_dtype (ridge_f = scales[idx], :138), may be
 * NULL when ridge_f is.  Outputs [batch][n_time][n_ridges]: ridge_idxs int64, ridge_f / ridge_e in param_dtype
 * (either may be NULL); cost_out [batch][n_ridges][n_freqs][n_time] in dtype, the cost each ridge tracked (:133),
 * NULL normally.  bw: the band zeroed around each ridge with Python slice rules (:141-143).  The backward trace is
 * upstream's serial one (:206-215); the `parallel` kernel (:217-232) races on ties and is not mirrored.
 * 1 <= n_freqs <= 32767, n_time >= 1, 1 <= batch <= 65535, n_ridges >= 1, bw >= 0.  Device pointers, async on
 * `stream`. */
int64_t ssq_ridges_workspace_bytes(int dtype, int64_t batch, int64_t n_freqs, int64_t n_time);
int ssq_ridges_exec(int dtype, int param_dtype, int is_complex, const void* d_Tf, int64_t batch, int64_t n_freqs,
                    int64_t n_time, const void* d_metric, const void* d_scales, double penalty, int64_t n_ridges,
                    double bw, int64_t* d_ridge_idxs, void* d_ridge_f, void* d_ridge_e, void* d_cost_out,
                    void* d_workspace, int64_t workspace_bytes, void* stream);
/* the same on host arrays (synchronous) */
int ssq_extract_ridges_host(int dtype, int param_dtype, int is_complex, const void* Tf, int64_t batch, int64_t n_freqs,
                            int64_t n_time, const void* metric, const void* scales, double penalty, int64_t n_ridges,
                            double bw, int64_t* ridge_idxs, void* ridge_f, void* ridge_e, void* cost_out);
/* fw_bw_ridge_tracking (:92-111) alone on a caller's cost [batch][n_freqs][n_time] in dtype: ridge_idxs [batch][n_time]
 * int64, pen_out [batch][n_freqs][n_time] the forward accumulated cost (:149-175), may be NULL.  Host arrays. */
int ssq_ridge_track_host(int dtype, int param_dtype, const void* cost, int64_t batch, int64_t n_freqs, int64_t n_time,
                         const void* metric, double penalty, int64_t* ridge_idxs, void* pen_out);

/* ---- component inversion: ssqueezepy.issq_cwt / issq_stft with cc, cw (old/ssqueezepy/_ssq_cwt.py:381-417) -----
 * Tx: [batch][rows][cols] complex of `dtype` (interleaved); cc, cw: [batch][cols][n_comp] int64, the layout of
 * ssq_ridges_exec's ridge_idxs, each value read as upstream's astype('int32') reads it (its low 32 bits); cw NULL:
 * cw_const everywhere.  For component k of column j the band is the rows clip(cc - cw, 0, rows) ..
 * clip(cc + cw, 0, rows) (int32 arithmetic) cut at rows - 1, empty where cc == -1.  x: [batch][n_comp + 1][cols]
 * float64, x[k] = scale * the sum of Re Tx over band k (bands may overlap: a row counts in every band holding it),
 * x[n_comp] = scale * the sum over the rows of no band; fp64 sums for both dtypes, in an order fixed by rows alone.
 * scale: 2 / adm_ssq(wavelet) (issq_cwt), 2 / window[n_fft / 2] (issq_stft).  1 <= n_comp <= 524280.
 * Device pointers, async on `stream`. */
int ssq_issq_components_exec(int dtype, const void* d_Tx, int64_t batch, int64_t rows, int64_t cols,
                             const int64_t* d_cc, const int64_t* d_cw, int64_t cw_const, int64_t n_comp, double scale,
                             double* d_x, void* stream);
/* the same on host arrays (synchronous); rejects a cc, cw or cw_const outside the int32 range */
int ssq_issq_components_host(int dtype, const void* Tx, int64_t batch, int64_t rows, int64_t cols, const int64_t* cc,
                             const int64_t* cw, int64_t cw_const, int64_t n_comp, double scale, double* x_out);

/* ---- synchrosqueezing of a given transform: ssqueezepy.phase_cwt / phase_stft / ssqueeze -------------------------
 * (old/ssqueezepy/algos.py:706-857, :126-252; ssqueezing.py:13-245).  Wx, dWx: [batch][rows][cols] complex of `dtype`
 * (interleaved); w: [batch][rows][cols] real of `dtype`; 1 <= rows <= 32767, 1 <= cols < 2^31.
 * Phase transform: w = |(B C - A D) / ((C^2 + D^2) 2 pi)| for Wx = C + iD, dWx = A + iB (STFT: Sfs given, [rows] real
 * of `dtype`: |Sfs[row] - ...|), +inf where |Wx| < gamma (a value is kept when |Wx| >= gamma, algos.py:724). */
int ssq_phase_exec(int dtype, const void* d_Wx, const void* d_dWx, const void* d_Sfs, int64_t batch, int64_t rows,
                   int64_t cols, double gamma, void* d_w, void* stream);
int ssq_phase_host(int dtype, const void* Wx, const void* dWx, const void* Sfs, int64_t batch, int64_t rows,
                   int64_t cols, double gamma, void* w);
/* ssqueeze only: squeezing 'abs' sums |Wx| into a real Tx (ssqueezing.py:185-186) */
enum { SSQ_SQUEEZE_ABS = 2 };
/* Squeeze from w (algos.py:153-252, `indexed_sum_onfly`): Tx[k, j] += Wx[i, j] * row_const[i] for every w[i, j] not
 * infinite, k by the bin rule of ssq_freqs_asc as for ssq_ssq_cwt_host_rows (freq_kind, freq_transition; clamped,
 * round half to even, k -> rows-1-k with flipud).  squeezing: SSQ_SQUEEZE_SUM (Tx complex), _LEBESGUE (Wx not read, may
 * be NULL: every row contributes 1/rows, Tx complex), _ABS (|Wx|, Tx real [batch][rows][cols]).  Tx is overwritten.
 * exec: d_row_const [rows] real of `dtype` on the device; ssq_freqs_asc [rows] fp64 on the host, read during the call
 * only.  host: row_const [rows] fp64, finite. */
int ssq_ssqueeze_w_exec(int dtype, const void* d_Wx, const void* d_w, int64_t batch, int64_t rows, int64_t cols,
                        const void* d_row_const, const double* ssq_freqs_asc, int freq_kind, int64_t freq_transition,
                        int squeezing, int flipud, void* d_Tx, void* stream);
int ssq_ssqueeze_w_host(int dtype, const void* Wx, const void* w, int64_t batch, int64_t rows, int64_t cols,
                        const double* row_const, const double* ssq_freqs_asc, int freq_kind, int64_t freq_transition,
                        int squeezing, int flipud, void* Tx);
/* Squeeze from dWx (algos.py:126-150, `ssqueeze_fast`): the phase transform, kept where |Wx| > gamma (algos.py:864),
 * binned and summed as above; squeezing SSQ_SQUEEZE_SUM or _LEBESGUE.  CWT (Sfs NULL): the fused ssq_cwt's
 * reassignment kernel, with the parameters of ssq_ssq_cwt_host_rows.  STFT (Sfs given): the fused upstream ssq_stft's,
 * freq_kind SSQ_FREQS_LINEAR, weight and bin width ssq_freqs_asc[1] - ssq_freqs_asc[0] (ssqueezing.py:129-130), the
 * first bin at Sfs[0], which must equal ssq_freqs_asc[0] (the host call checks it); row_const is not read, batch <= 65535.
 * Tx: [batch][rows][cols] complex, overwritten. */
int ssq_ssqueeze_dwx_exec(int dtype, const void* d_Wx, const void* d_dWx, const void* d_Sfs, int64_t batch,
                          int64_t rows, int64_t cols, const void* d_row_const, const double* ssq_freqs_asc,
                          int freq_kind, int64_t freq_transition, int squeezing, int flipud, double gamma, void* d_Tx,
                          void* stream);
int ssq_ssqueeze_dwx_host(int dtype, const void* Wx, const void* dWx, const void* Sfs, int64_t batch, int64_t rows,
                          int64_t cols, const double* row_const, const double* ssq_freqs_asc, int freq_kind,
                          int64_t freq_transition, int squeezing, int flipud, double gamma, void* Tx);

/* ---- multi-GPU: the optional final gather of the batch-sharded results over xGMI ------------------------------
 * Signals are independent (the reference's batch is a Python loop over channels, tests/stft_ssq_test.py:230), so the
 * data path has no collective; a consumer that wants every rank to hold all shards calls ssq_gather_shards after its
 * plan exec.  RCCL (librccl.so) is dlopen'd on first use -- no link-time dependency, a clear error when absent.
 * One process per GPU: rank 0 makes the 128-byte id (ssq_rccl_unique_id) and hands it to the others out of band
 * (MPI, a file, torch.distributed, ...); every rank then calls ssq_rccl_comm_init on its own device.  `comm` may also
 * be a ncclComm_t the caller created itself. */
int ssq_rccl_available(void);                                 /* 1 if librccl.so loads */
int ssq_rccl_unique_id(void* id128);                          /* ncclGetUniqueId */
int ssq_rccl_comm_init(void** comm, int n_ranks, const void* id128, int rank);   /* ncclCommInitRank (collective) */
int ssq_rccl_comm_info(void* comm, int* n_ranks, int* rank);  /* ncclCommCount / ncclCommUserRank */
int ssq_rccl_comm_destroy(void* comm);
/* ncclAllGather of `bytes_per_rank` bytes: d_recv[rank][bytes_per_rank], rank order = batch order; async on `stream` */
int ssq_gather_shards(void* comm, const void* d_send, void* d_recv, int64_t bytes_per_rank, void* stream);

/* ---- host-path caches ---------------------------------------------------------
 * The *_host entry points keep plans (keyed by their configuration), device scratch and two streams between
 * calls, and pipeline H2D / kernels / D2H over the signals of a batch.  Results that live in blocks of the
 * library's pinned pool arrive by DMA without a host-side copy; `ssqueeze_rs_amd._rs` allocates its NumPy results
 * there (the reference hands NumPy freshly allocated arrays too: ssq_stft.rs:307-312). */
int ssq_pinned_alloc(void** ptr, int64_t bytes);         /* pooled hipHostMalloc */
int ssq_pinned_free(void* ptr);                          /* back to the pool */
int ssq_host_cache_limit(int64_t idle_pinned_bytes);     /* idle pinned memory the pool may keep (default 8 GiB) */
int ssq_host_cache_stats(int64_t* live_pinned_bytes, int64_t* idle_pinned_bytes);
/* An aid for testing the host slices: at most `signals` signals per slice in every synchronous *_host entry point that
 * slices a batch to fit device memory (0, the default: no cap; negative: an error).  Process-wide; results do not
 * depend on it. */
int ssq_host_slice_cap(int64_t signals);
int ssq_host_cache_clear(void);                          /* drop cached plans, device scratch, idle pinned blocks */

/* ---- device memory / stream / event plumbing for FFI callers --------------- */
int ssq_dev_malloc(void** ptr, int64_t bytes);
int ssq_dev_free(void* ptr);
int ssq_dev_memset(void* ptr, int value, int64_t bytes, void* stream);
int ssq_memcpy_h2d(void* dst, const void* src, int64_t bytes, void* stream);
int ssq_memcpy_d2h(void* dst, const void* src, int64_t bytes, void* stream);
int ssq_memcpy_d2d(void* dst, const void* src, int64_t bytes, void* stream);
int ssq_stream_create(void** stream);
int ssq_stream_destroy(void* stream);
int ssq_stream_sync(void* stream);     /* NULL = default stream */
int ssq_device_sync(void);
int ssq_event_create(void** event);
int ssq_event_destroy(void* event);
int ssq_event_record(void* event, void* stream);
int ssq_event_sync(void* event);
int ssq_event_elapsed_ms(void* start, void* stop, float* ms);
/* HIP graphs: everything the plan execs enqueue on `stream` between begin and end (incl. the ssq_cwt exec's side-stream
 * fork / join) becomes ONE replayable launch.  Run the sequence once before capturing (lazy one-time setup in the plans);
 * replay with the same device pointers (new contents).  `stream` must be an explicit stream (ssq_stream_create). */
int ssq_graph_capture_begin(void* stream);
int ssq_graph_capture_end(void* stream, void** graph_exec);
int ssq_graph_launch(void* graph_exec, void* stream);
int ssq_graph_destroy(void* graph_exec);

#ifdef __cplusplus
}
#endif
#endif /* SSQ_HIP_H */
