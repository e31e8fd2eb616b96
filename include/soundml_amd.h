/*
 * soundml_amd.h -- C ABI of the MI355X-native spectral path for SoundML.
 *
 * This is the drop-in boundary: plain C, raw pointers + int64 extents, an int
 * status and a thread-local error string.  Each entry point names the reference
 * interface it replaces (paths relative to /root/reference/soundml/lib).  The
 * OCaml side binds these with `external` + CAMLprim stubs exactly like the
 * reference binds resample_stubs.c (resample.ml:1162-1196); see INTEGRATION.md
 * and ocaml/soundml_amd_stubs.c.
 *
 * Conventions (reference: soundml.mli:3-24, stft.mli:211-250)
 *   - time axis last; audio is [lead; n], spectra are [lead; bins; frames]
 *     (frames fastest); `lead` is the product of all leading axes;
 *   - inputs are borrowed for the call, outputs are caller-allocated and fully
 *     overwritten, nothing is retained (stft.mli:454-458);
 *   - complex outputs are interleaved (re, im) pairs of the component type;
 *   - user-facing precondition failures return SMX_INVALID_ARGUMENT with the
 *     reference's own message (OCaml: raise Invalid_argument); geometry /
 *     runtime (HIP) failures return SMX_FAILURE (OCaml: Failure);
 *   - `*_dev` entry points take DEVICE pointers on the current HIP device and a
 *     hipStream_t (as void*); they enqueue work and return without
 *     synchronising.  The host-pointer entry points upload, run and download
 *     (this is what an nx-tensor caller uses).
 *   - streams: every launch, memset, copy and scratch array of a call is ordered
 *     on the caller's stream and on no other; only the entry points that say so
 *     (the spectral-shape features and the flat spectral contrast of a
 *     spectrogram, which read one flag back) wait for it, and they return with
 *     it idle; configurations may be shared between streams.  The first use of
 *     a configuration builds its tables with blocking copies
 *     (tests/test_gpu_streams.py).
 *   - placement of the `*_dev` buffers: any pointer aligned to its element type
 *     (float: 4 bytes, double and complex64: 8, complex128: 16) is valid -- no
 *     entry point asks for more; a row stride is in elements and >= the row's
 *     length n; what lies between the rows, before the first and behind the
 *     last one is the caller's: it is neither read into a result nor written
 *     (tests/test_gpu_placement.py).
 *   - every extent is validated before any pointer is formed or any device
 *     work is enqueued (discipline of resample_stubs.c:228-276).
 *   - the library never falls back to a CPU implementation: without a HIP
 *     device every compute entry point returns SMX_FAILURE.
 */
#ifndef SOUNDML_AMD_H
#define SOUNDML_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMX_OK 0
#define SMX_INVALID_ARGUMENT 1
#define SMX_FAILURE 2

/* "argument not given" for optional integer arguments (OCaml ?win_length / ?hop) */
#define SMX_DEFAULT INT64_MIN

/* Stft.Config.alignment (stft.ml:53) */
#define SMX_ALIGN_CENTERED 0
#define SMX_ALIGN_LEFT 1
#define SMX_ALIGN_RIGHT 2
/* Stft.Config.pad (stft.ml:54) */
#define SMX_PAD_REFLECT 0
#define SMX_PAD_CONSTANT 1
#define SMX_PAD_EDGE 2
/* Stft.Config.scale (stft.ml:55) */
#define SMX_SCALE_NONE 0
#define SMX_SCALE_MAGNITUDE 1
#define SMX_SCALE_PSD 2
/* Window.t families built by the library (window.ml:362-375); any other family
 * is built by the host in float64 and passed as a table (SMX_WINDOW_CUSTOM). */
#define SMX_WINDOW_HANN 0
#define SMX_WINDOW_RECTANGULAR 1
#define SMX_WINDOW_HAMMING 2
#define SMX_WINDOW_BLACKMAN 3
#define SMX_WINDOW_BLACKMAN_HARRIS 4
#define SMX_WINDOW_NUTTALL 5
#define SMX_WINDOW_FLAT_TOP 6
#define SMX_WINDOW_BARTLETT 7
#define SMX_WINDOW_KAISER 8      /* shape parameter: beta, finite and non-negative      */
#define SMX_WINDOW_GAUSSIAN 9    /* shape parameter: standard deviation in samples, > 0 */
#define SMX_WINDOW_TUKEY 10      /* shape parameter: taper fraction in [0, 1]           */
#define SMX_WINDOW_CUSTOM 100
/* Mel.Config.scale / norm (mel.ml:26-27) */
#define SMX_MEL_SLANEY 0
#define SMX_MEL_HTK 1
#define SMX_NORM_SLANEY 0
#define SMX_NORM_NONE 1
/* Interior arithmetic for float32 audio.  The reference computes in float64
 * whatever the I/O dtype (stft.ml:28-35); SMX_INTERIOR_F32 is the documented
 * fast deviation (north_star: 1e-5 relative), SMX_INTERIOR_F64 reproduces the
 * reference's interior (widen, f64 window multiply, f64 FFT, one rounding).
 * float64 audio always uses the float64 interior. */
#define SMX_INTERIOR_F32 0
#define SMX_INTERIOR_F64 1
/* Resample.quality (resample.ml:519-526): 100 / 126 / 175 dB at passband 0.913, or `Custom {attenuation; passband} */
#define SMX_RESAMPLE_FAST 0
#define SMX_RESAMPLE_HIGH 1
#define SMX_RESAMPLE_BEST 2
#define SMX_RESAMPLE_CUSTOM 3
/* what runs the one stage of a Resample.Config (smx_resample_config_executor) */
#define SMX_RESAMPLE_IDENTITY 0
#define SMX_RESAMPLE_OLS 1
#define SMX_RESAMPLE_DIRECT 2

typedef struct smx_stft_config smx_stft_config;
typedef struct smx_mel_config smx_mel_config;
typedef struct smx_chroma_config smx_chroma_config;
typedef struct smx_stft_kernel smx_stft_kernel;
typedef struct smx_fir_plan smx_fir_plan;
typedef struct smx_resample_stage smx_resample_stage;
typedef struct smx_resample_kernel smx_resample_kernel;
typedef struct smx_resample_config smx_resample_config;
typedef struct smx_resample_stream smx_resample_stream;

/* ---- library ------------------------------------------------------------ */
const char *smx_last_error(void);      /* message of the last failing call on this thread */
int smx_version(void);
/* diagnostics: kernel launches issued by this process through the library so far (bench.py asserts that one step
 * of the hot path is one launch, so that HIP events around a step time that kernel) */
unsigned long long smx_debug_kernel_launches(void);
/* diagnostics (tests of Griffin-Lim's internal layout): Stft.transform of device-resident float32 audio at fft 2048 with the
 * spectrum FRAME-MAJOR -- out[clip][frame][bin] complex64 in rows of pitch_floats floats, rows_per_clip (the frames rounded up to
 * a multiple of 16) rows per clip; fails where the frame-major kernel does not apply */
int smx_debug_stft_transform_frame_major_f32_dev(const smx_stft_config *c, const float *d_x, int64_t lead, int64_t n, float *d_out,
                                                 int64_t pitch_floats, int64_t rows_per_clip, void *stream);
int smx_device_count(int *count);
int smx_set_device(int device);        /* device used by this thread's subsequent calls */
/* Clip sharding for the HOST-POINTER batch calls (round 6).  The reference's caller is one process that hands over host
 * tensors, "a batch of clips is one call" (stft.mli:211-250, soundml.mli:3-24), and its leading axes are independent by contract
 * (stft.mli:214-218; per-slice law tested in stft_grid.ml:180-205, mel_props.ml:136-155).  With a device list set, every
 * host-pointer entry point of Stft.transform / transform_range / power_spectrum / power_range / invert and
 * Soundml.mel_spectrogram splits `lead` into contiguous clip ranges -- shard s of S owns clips [s*q + min(s, r), ...) with
 * q = lead / S, r = lead % S, the first r shards one clip more (soundml_amd/shard.py clip_range) -- and runs each range on its
 * device from a host thread of its own, with that device's own staging rings and PCIe link; every shard writes its slice of the
 * caller's `out`, so the result is the single-device call's bit for bit and no collective is involved.  A device may be listed
 * more than once (virtual shards).  n = 0 clears the list: calls run on the calling thread's current device (smx_set_device).
 * Process-wide; the `*_dev` entry points and the streaming states are not affected (they live on one device by construction).
 * smx_get_devices writes min(*n, capacity) ordinals. */
int smx_set_devices(const int *devices, int n);
int smx_get_devices(int *devices, int capacity, int *n);
/* the rule itself (no device needed): clips [*lo, *hi) of shard `shard` of `shards` -- what a caller that gathers per-device results
 * itself, or a test, checks the split against (soundml_amd/shard.py clip_range is the same function) */
int smx_shard_clip_range(int64_t total_clips, int64_t shards, int64_t shard, int64_t *lo, int64_t *hi);
/* diagnostics (tests of the per-device staging): the most staged uploads / downloads that were ever in flight at once */
int smx_debug_staging_peak(int *uploads, int *downloads, int reset);
/* diagnostics (tests of the launch extents; no device needed): one launch holds at most 2^32 - 1 work-items and 2^31 - 1 workgroups
 * on its first grid axis, so a batch whose clips each take `tiles_per_clip` workgroups of `threads` goes this many clips at a time
 * (0: a single clip does not fit, which the entry point refuses with "too many ... for one launch") */
int64_t smx_debug_clips_per_launch(int64_t tiles_per_clip, int threads);
int smx_set_interior(int interior);    /* SMX_INTERIOR_*, process-wide default for f32 audio */
/* Scratch arrays (Griffin-Lim's spectra, scratch spectrograms, small tables) come from a stream-ordered memory pool
 * that the library creates for itself on each device (the process-wide default pool is never touched); it keeps up to
 * `bytes` of freed scratch per device for reuse instead of returning it to the driver at every synchronisation
 * (default: 1/8 of the device's memory, at most 16 GiB; 0 = keep nothing; -1 = the default again).  Memory held this
 * way is not visible to another allocator in the process (e.g. torch's): lower it when embedding. */
int smx_set_scratch_retention(int64_t bytes);
int smx_get_interior(void);
int smx_synchronize(void *stream);
/* Result arrays for the host-pointer entry points.  The reference's faces return a fresh host tensor per call (`analyse`
 * allocates its result inside Nx.stft: stft.ml:356-364; Stft.power_spectrum: stft.ml:670-691).  Fresh pageable memory is the slow
 * half of such a call -- every page of a 0.98 GB spectrogram faults as the copying threads reach it, and the bytes cross host
 * memory twice (DMA into a staging ring, then memcpy).  A block from smx_host_alloc is page-locked: when the `out` (or `x`)
 * pointer of a host-pointer entry point lies inside one, the DMA engine writes (reads) it directly.  smx_host_free returns the
 * block to the library, which keeps up to 3 GiB of released blocks for the next result of about the same size.  A binding
 * allocates its result tensors here (the OCaml stub wraps the block in a Bigarray whose finaliser calls smx_host_free:
 * INTEGRATION.md section 2); a pointer from any other allocator takes the staged path, as before.  Thread-safe. */
int smx_host_alloc(size_t bytes, void **ptr);
int smx_host_free(void *ptr);

/* ---- Window.make (window.ml:374-405), float64, Hann & friends ------------ */
int smx_window_make(int kind, int periodic, int64_t n, double *out);
/* the parametric families too (window.ml:77-97 validate their shape parameter; ignored by the others) */
int smx_window_make_param(int kind, double param, int periodic, int64_t n, double *out);
/* Window.cola (window.ml:407-434): 1 iff the `length`-point periodic window overlap-adds to a constant at `hop` */
int smx_window_cola(int kind, double param, int64_t length, int64_t hop, int *cola);

/* ---- Stft.Config (stft.ml:48-129) --------------------------------------- */
int smx_stft_config_create(int64_t fft_size, int64_t win_length /* SMX_DEFAULT = fft_size */,
                           int64_t hop /* SMX_DEFAULT = max 1 (fft_size/4) */, int alignment,
                           int pad, double pad_value, int scale, int window_kind,
                           const double *custom_window /* win_length doubles iff SMX_WINDOW_CUSTOM */,
                           smx_stft_config **out);
void smx_stft_config_destroy(smx_stft_config *c);
int64_t smx_stft_config_fft_size(const smx_stft_config *c);
int64_t smx_stft_config_hop(const smx_stft_config *c);
int64_t smx_stft_config_win_length(const smx_stft_config *c);
int64_t smx_stft_config_bins(const smx_stft_config *c);          /* stft.ml:127 */
int64_t smx_stft_config_left_width(const smx_stft_config *c);    /* stft.ml:132-140 */
int64_t smx_stft_config_right_width(const smx_stft_config *c);   /* stft.ml:141-142 */
int64_t smx_stft_config_latency(const smx_stft_config *c);       /* stft.ml:144-145 */
int smx_stft_config_analysis_window(const smx_stft_config *c, double *out /* fft_size */);

/* ---- frame grid (stft.ml:217-261) ---------------------------------------- */
int smx_stft_frames(const smx_stft_config *c, int64_t n, int64_t *out);
int smx_stft_first_complete(const smx_stft_config *c, int64_t *out);
int smx_stft_last_complete(const smx_stft_config *c, int64_t n, int64_t *out);
int smx_stft_times(const smx_stft_config *c, int64_t sample_rate, int64_t n, double *out /* frames */);
int smx_stft_frequencies(const smx_stft_config *c, int64_t sample_rate, double *out /* bins */);

/* ---- Stft.transform / transform_range / power_spectrum (stft.ml:632-691) ---
 * x: [lead; n] contiguous (x_stride = elements between consecutive signals, >= n).
 * out: transform -> complex [lead; bins; frames]; range -> [lead; bins; p1-p0];
 *      power_spectrum -> real [lead; bins; frames].                           */
int smx_stft_transform_f32(const smx_stft_config *c, const float *x, int64_t lead, int64_t n,
                           float *out_c64);
int smx_stft_transform_f64(const smx_stft_config *c, const double *x, int64_t lead, int64_t n,
                           double *out_c128);
int smx_stft_transform_range_f32(const smx_stft_config *c, const float *x, int64_t lead, int64_t n,
                                 int64_t p0, int64_t p1, float *out_c64);
int smx_stft_transform_range_f64(const smx_stft_config *c, const double *x, int64_t lead, int64_t n,
                                 int64_t p0, int64_t p1, double *out_c128);
int smx_stft_power_spectrum_f32(const smx_stft_config *c, const float *x, int64_t lead, int64_t n,
                                double power, float *out);
int smx_stft_power_spectrum_f64(const smx_stft_config *c, const double *x, int64_t lead, int64_t n,
                                double power, double *out);
/* |frames [p0, p1)|^power: transform_range (stft.ml:652-666) followed by magnitude_pow (stft.ml:670-674) */
int smx_stft_power_range_f32(const smx_stft_config *c, const float *x, int64_t lead, int64_t n, int64_t p0,
                             int64_t p1, double power, float *out);
int smx_stft_power_range_f64(const smx_stft_config *c, const double *x, int64_t lead, int64_t n, int64_t p0,
                             int64_t p1, double power, double *out);
/* device-resident forms (the batch API the benchmark and the sharded driver use) */
int smx_stft_transform_range_f32_dev(const smx_stft_config *c, const float *d_x, int64_t lead,
                                     int64_t n, int64_t x_stride, int64_t p0, int64_t p1,
                                     float *d_out_c64, void *stream);
int smx_stft_transform_range_f64_dev(const smx_stft_config *c, const double *d_x, int64_t lead,
                                     int64_t n, int64_t x_stride, int64_t p0, int64_t p1,
                                     double *d_out_c128, void *stream);
int smx_stft_power_range_f32_dev(const smx_stft_config *c, const float *d_x, int64_t lead,
                                 int64_t n, int64_t x_stride, int64_t p0, int64_t p1, double power,
                                 float *d_out, void *stream);
int smx_stft_power_range_f64_dev(const smx_stft_config *c, const double *d_x, int64_t lead,
                                 int64_t n, int64_t x_stride, int64_t p0, int64_t p1, double power,
                                 double *d_out, void *stream);

/* ---- Stft.Kernel (stft.ml:597-622): streaming analysis, device-resident carry
 * dtype_bytes: 4 (float32 audio, complex64 spectra) or 8.
 * step/flush write at most `capacity` frames into out [channels; bins; capacity]
 * laid out with `capacity` as the frame stride, and report how many they emitted
 * (0 = the reference's None).  frame_bound = stft.ml:1316-1317.               */
int smx_stft_kernel_prepare(const smx_stft_config *c, int dtype_bytes, int64_t channels,
                            int64_t max_block, smx_stft_kernel **out);
/* the same state machine emitting |spectrum|^power in the chunk's dtype ([channels; bins; capacity] real): the body
 * of Stft.power_stage (stft.ml:1364-1409); stage_latency / frame_bound / stage_rate of stft.ml:1307-1348 are
 * smx_stft_stage_latency, smx_stft_frame_bound and 1 / hop.                                                   */
int smx_stft_kernel_prepare_power(const smx_stft_config *c, int dtype_bytes, int64_t channels, int64_t max_block,
                                  double power, smx_stft_kernel **out);
int64_t smx_stft_stage_latency(const smx_stft_config *c);                 /* stft.ml:1307-1308 */
int64_t smx_stft_frame_bound(const smx_stft_config *c, int64_t max_items); /* stft.ml:1316-1317 */
void smx_stft_kernel_destroy(smx_stft_kernel *k);
int smx_stft_kernel_frame_bound(const smx_stft_kernel *k, int64_t *out);
int smx_stft_kernel_step(smx_stft_kernel *k, const void *chunk /* host [channels; m] */, int64_t m,
                         void *out_complex, int64_t capacity, int64_t *emitted);
int smx_stft_kernel_flush(smx_stft_kernel *k, void *out_complex, int64_t capacity, int64_t *emitted);
int smx_stft_kernel_reset(smx_stft_kernel *k);
/* the same state machine fed from and emitting into DEVICE memory (chunk rows x_stride samples apart; the window
 * [channels; bins; capacity] as above): a push moves nothing over the host link.  The frame count comes back on the host
 * (it is bookkeeping of lengths, known before any kernel runs); the frames are ready in stream order.                */
int smx_stft_kernel_step_dev(smx_stft_kernel *k, const void *d_chunk, int64_t m, int64_t x_stride, void *d_out,
                             int64_t capacity, int64_t *emitted, void *stream);
int smx_stft_kernel_flush_dev(smx_stft_kernel *k, void *d_out, int64_t capacity, int64_t *emitted, void *stream);
/* The reference's state takes its leading shape from the chunks it is fed (stft.ml:521-559: only `channels >= 1` is checked
 * at prepare, stft.ml:603-617), so a binding must be able to follow the first chunk: channels() reports the count the
 * kernel was prepared for (step / flush read and write exactly that many rows: a caller passes buffers of that extent),
 * set_channels() re-shapes a kernel that has not received a sample since prepare / reset and refuses one that has
 * (SMX_INVALID_ARGUMENT: the stream's chunks disagree in their leading shape).                                      */
int smx_stft_kernel_channels(const smx_stft_kernel *k, int64_t *out);
int smx_stft_kernel_set_channels(smx_stft_kernel *k, int64_t channels);
const smx_stft_config *smx_stft_kernel_config(const smx_stft_kernel *k);   /* the configuration it was prepared with (borrowed) */

/* ---- Stft.Synthesis (stft.ml:1271-1298; stft.mli:519-591) and the body of synthesis_stage (stft.ml:1417-1442):
 * incremental least-squares synthesis with the state in device memory.  dtype_bytes 4: complex64 frames in, float32
 * samples out; 8: complex128 / float64.  step takes k frames [channels; bins; k] (frames fastest) and releases every sample
 * they settle into out [channels; capacity] (row stride = capacity), reporting how many per channel (0 = the reference's
 * None); flush drains the trimmed tail.  Any chunking of a stream totals smx_stft_invert of the whole stream, bit for
 * bit.  sample_bound = the most samples one step of max_block frames or the flush can release (synthesis_stage's
 * max_items, stft.ml:1421-1427); smx_stft_synthesis_latency = Config.synthesis_latency (stft.ml:152-153).            */
typedef struct smx_stft_synthesis smx_stft_synthesis;
int smx_stft_synthesis_prepare(const smx_stft_config *c, int dtype_bytes, int64_t channels, int64_t max_block,
                               smx_stft_synthesis **out);
void smx_stft_synthesis_destroy(smx_stft_synthesis *s);
int64_t smx_stft_synthesis_latency(const smx_stft_config *c);
int smx_stft_synthesis_sample_bound(const smx_stft_synthesis *s, int64_t *out);
int smx_stft_synthesis_step(smx_stft_synthesis *s, const void *z, int64_t bins, int64_t k, void *out, int64_t capacity,
                            int64_t *emitted);
int smx_stft_synthesis_flush(smx_stft_synthesis *s, void *out, int64_t capacity, int64_t *emitted);
int smx_stft_synthesis_reset(smx_stft_synthesis *s);
/* the same on device-resident chunks and outputs (no host copy per push) */
int smx_stft_synthesis_step_dev(smx_stft_synthesis *s, const void *d_z, int64_t bins, int64_t k, void *d_out,
                                int64_t capacity, int64_t *emitted, void *stream);
int smx_stft_synthesis_flush_dev(smx_stft_synthesis *s, void *d_out, int64_t capacity, int64_t *emitted, void *stream);

/* ---- Mel.Config / Mel.apply (mel.ml:22-233) ------------------------------- */
/* Convert.hz_to_mel / mel_to_hz (convert.ml:70-102): the scalar maps behind the filterbank's breakpoints; host float64 */
int smx_hz_to_mel(int scale /* SMX_MEL_* */, const double *f, int64_t n, double *out);
int smx_mel_to_hz(int scale, const double *m, int64_t n, double *out);
int smx_mel_config_create(int64_t n_mels, int64_t sample_rate, int64_t fft_size, double f_min,
                          int has_f_max, double f_max, int scale, int norm, smx_mel_config **out);
/* A filterbank handle over caller-supplied float64 weights [rows; fft_size/2 + 1] (copied): every projection of
 * the reference that is `matmul W (power spectrum)` with its own W -- Chroma.apply's chroma filters
 * (chroma.ml:307), a mel bank built elsewhere -- runs through smx_mel_apply_* / smx_mel_spectrogram_*.       */
int smx_mel_config_from_weights(int64_t rows, int64_t fft_size, const double *weights, smx_mel_config **out);
void smx_mel_config_destroy(smx_mel_config *c);
int64_t smx_mel_config_n_mels(const smx_mel_config *c);
int64_t smx_mel_config_bins(const smx_mel_config *c);
int64_t smx_mel_config_fft_size(const smx_mel_config *c);
double smx_mel_config_f_max(const smx_mel_config *c);
int smx_mel_filterbank(const smx_mel_config *c, double *out /* [n_mels; bins] */); /* mel.ml:200 */
/* s: [lead; bins; frames] -> out [lead; n_mels; frames]; `bins` is the caller's
 * declared axis size and is checked against the config (mel.ml:210-218).     */
int smx_mel_apply_f32(const smx_mel_config *c, const float *s, int64_t lead, int64_t bins,
                      int64_t frames, float *out);
int smx_mel_apply_f64(const smx_mel_config *c, const double *s, int64_t lead, int64_t bins,
                      int64_t frames, double *out);
int smx_mel_apply_f32_dev(const smx_mel_config *c, const float *d_s, int64_t lead, int64_t bins,
                          int64_t frames, float *d_out, void *stream);
int smx_mel_apply_f64_dev(const smx_mel_config *c, const double *d_s, int64_t lead, int64_t bins,
                          int64_t frames, double *d_out, void *stream);

/* ---- Soundml.mel_spectrogram (soundml.ml:12-24): fused audio -> mel -------- */
int smx_mel_spectrogram_f32(const smx_stft_config *sc, const smx_mel_config *mc, const float *x,
                            int64_t lead, int64_t n, double power, float *out);
int smx_mel_spectrogram_f64(const smx_stft_config *sc, const smx_mel_config *mc, const double *x,
                            int64_t lead, int64_t n, double power, double *out);
int smx_mel_spectrogram_f32_dev(const smx_stft_config *sc, const smx_mel_config *mc,
                                const float *d_x, int64_t lead, int64_t n, int64_t x_stride,
                                double power, float *d_out, void *stream);

/* ---- Stft.griffin_lim (stft.ml:941-1017): phase reconstruction from magnitudes s [lead; bins; frames].
 * c_k = analyse (synthesise (s * angles_k)),  angles_{k+1} = unit (c_k - a c_{k-1}),  a = momentum / (1 + momentum);
 * the loop runs at the natural length, `length` applies to the final synthesis only.  init_phase (radians,
 * same shape) or NULL for the all-ones phase.  out is [lead; out_len] as for smx_stft_invert_*.
 * Invalid_argument: the synthesis checks, n_iter < 1, momentum < 0 (messages of stft.ml:963-976).           */
int smx_stft_griffin_lim_f32(const smx_stft_config *c, const float *s, int64_t lead, int64_t bins, int64_t frames,
                             int64_t n_iter, double momentum, const float *init_phase, int has_length,
                             int64_t length, float *out);
int smx_stft_griffin_lim_f64(const smx_stft_config *c, const double *s, int64_t lead, int64_t bins, int64_t frames,
                             int64_t n_iter, double momentum, const double *init_phase, int has_length,
                             int64_t length, double *out);
int smx_stft_griffin_lim_f32_dev(const smx_stft_config *c, const float *d_s, int64_t lead, int64_t bins,
                                 int64_t frames, int64_t n_iter, double momentum, const float *d_init_phase,
                                 int has_length, int64_t length, float *d_out, void *stream);

/* ---- Convert.power_to_db / amplitude_to_db (convert.ml:30-62): decibels in the data's own dtype -------
 * db = scale * ln(max(v, amin)) - scale * ln(max(amin, reference)), scale = gain / ln 10 (gain 10 for powers, 20 for
 * amplitudes, which take |s| first: a negative power sits at the floor); with has_top_db the result is clamped at
 * (the maximum over the WHOLE tensor) - top_db.  `total` elements of any shape; out may alias s on the device.
 * Invalid_argument (convert.ml:3-16): reference / amin not finite and positive, top_db negative or not finite. */
int smx_power_to_db_f32(const float *s, int64_t total, double reference, double amin, int has_top_db, double top_db,
                        float *out);
int smx_power_to_db_f64(const double *s, int64_t total, double reference, double amin, int has_top_db, double top_db,
                        double *out);
int smx_power_to_db_f32_dev(const float *d_s, int64_t total, double reference, double amin, int has_top_db,
                            double top_db, float *d_out, void *stream);
int smx_amplitude_to_db_f32(const float *s, int64_t total, double reference, double amin, int has_top_db,
                            double top_db, float *out);
int smx_amplitude_to_db_f64(const double *s, int64_t total, double reference, double amin, int has_top_db,
                            double top_db, double *out);
int smx_amplitude_to_db_f32_dev(const float *d_s, int64_t total, double reference, double amin, int has_top_db,
                                double top_db, float *d_out, void *stream);

/* ---- Convert.db_to_power / db_to_amplitude (convert.ml:58-68): reference * 10^(db / 10) and reference * 10^(db / 20),
 * evaluated in float64 and rounded once to the data's dtype.  `total` elements of any shape; out may alias db on the
 * device.  Invalid_argument (convert.ml:3-6): reference not finite and positive.                                 */
int smx_db_to_power_f32(const float *db, int64_t total, double reference, float *out);
int smx_db_to_power_f64(const double *db, int64_t total, double reference, double *out);
int smx_db_to_power_f32_dev(const float *d_db, int64_t total, double reference, float *d_out, void *stream);
int smx_db_to_power_f64_dev(const double *d_db, int64_t total, double reference, double *d_out, void *stream);
int smx_db_to_amplitude_f32(const float *db, int64_t total, double reference, float *out);
int smx_db_to_amplitude_f64(const double *db, int64_t total, double reference, double *out);
int smx_db_to_amplitude_f32_dev(const float *d_db, int64_t total, double reference, float *d_out, void *stream);
int smx_db_to_amplitude_f64_dev(const double *d_db, int64_t total, double reference, double *d_out, void *stream);
/* Convert.hz_to_midi / midi_to_hz (convert.ml:104-106): 12 log2 (f / 440) + 69 and back; host float64 */
int smx_hz_to_midi(const double *f, int64_t n, double *out);
int smx_midi_to_hz(const double *m, int64_t n, double *out);
/* Convert.frames_to_time / time_to_frames (convert.ml:108-115): frames * hop / sample_rate, and floor (times *
 * sample_rate / hop); host float64.  Invalid_argument (convert.ml:18-20): sample_rate < 1, hop < 1.           */
int smx_frames_to_time(int64_t sample_rate, int64_t hop, const double *frames, int64_t n, double *out);
int smx_time_to_frames(int64_t sample_rate, int64_t hop, const double *times, int64_t n, double *out);

/* ---- Mel.invert (DESIGN.md "Mel inversion"): m [lead; n_mels; frames] -> out [lead; bins; frames], per frame the
 * non-negative s that approaches min |W s - m|_2 after n_iter rounds of accelerated projected gradient from zero, in
 * the data's dtype, all rounds inside one launch.  power = 1: s itself; otherwise s^(1 / power) in float64 rounded once
 * (mel_to_stft: the magnitudes behind a spectrogram raised to `power`; power 2 is a square root).
 * Invalid_argument: a handle of smx_mel_config_from_weights, n_mels != the config's, n_iter < 0, power not finite and
 * positive.                                                                                                     */
int smx_mel_invert_f32(const smx_mel_config *c, const float *m, int64_t lead, int64_t n_mels, int64_t frames,
                       int64_t n_iter, double power, float *out);
int smx_mel_invert_f64(const smx_mel_config *c, const double *m, int64_t lead, int64_t n_mels, int64_t frames,
                       int64_t n_iter, double power, double *out);
int smx_mel_invert_f32_dev(const smx_mel_config *c, const float *d_m, int64_t lead, int64_t n_mels, int64_t frames,
                           int64_t n_iter, double power, float *d_out, void *stream);
int smx_mel_invert_f64_dev(const smx_mel_config *c, const double *d_m, int64_t lead, int64_t n_mels, int64_t frames,
                           int64_t n_iter, double power, double *d_out, void *stream);

/* ---- mfcc_to_mel: the tail of Soundml.mfcc backwards (soundml.ml:26-95; DESIGN.md "Mel inversion"): row k divided by
 * its lifter weight 1 + (lifter / 2) sin (pi (k + 1) / lifter), the cepstral axis zero-padded to n_mels, the inverse of
 * the orthonormal DCT-II along it, then reference * 10^(db / 10); float64 inside, one rounding.
 * c [lead; n_mfcc; frames] -> out [lead; n_mels; frames].  Invalid_argument: n_mels < n_mfcc, n_mfcc < 1, lifter
 * negative or not finite, a lifter weight of exactly zero, reference not finite and positive.                   */
int smx_mfcc_to_mel_f32(const float *c, int64_t lead, int64_t n_mfcc, int64_t frames, int64_t n_mels, int has_lifter,
                        double lifter, double reference, float *out);
int smx_mfcc_to_mel_f64(const double *c, int64_t lead, int64_t n_mfcc, int64_t frames, int64_t n_mels, int has_lifter,
                        double lifter, double reference, double *out);
int smx_mfcc_to_mel_f32_dev(const float *d_c, int64_t lead, int64_t n_mfcc, int64_t frames, int64_t n_mels,
                            int has_lifter, double lifter, double reference, float *d_out, void *stream);
int smx_mfcc_to_mel_f64_dev(const double *d_c, int64_t lead, int64_t n_mfcc, int64_t frames, int64_t n_mels,
                            int has_lifter, double lifter, double reference, double *d_out, void *stream);

/* ---- Soundml.mfcc (soundml.ml:50-95): mel_spectrogram (power 2) -> power_to_db with the 80 dB clamp under
 * the maximum of the WHOLE tensor (convert.ml:30-50) -> orthonormal DCT-II along the mel axis, first n_mfcc
 * rows -> optional sinusoidal lifter.  float64 interior after the mel spectrogram, one rounding to the audio
 * dtype.  out is [lead; n_mfcc; frames].  Invalid_argument: fft sizes differ, n_mfcc outside [1, n_mels],
 * lifter negative or not finite (messages of soundml.ml:52-70).                                          */
int smx_mfcc_f32(const smx_stft_config *sc, const smx_mel_config *mc, const float *x, int64_t lead, int64_t n,
                 int64_t n_mfcc, int has_lifter, double lifter, float *out);
int smx_mfcc_f64(const smx_stft_config *sc, const smx_mel_config *mc, const double *x, int64_t lead, int64_t n,
                 int64_t n_mfcc, int has_lifter, double lifter, double *out);
int smx_mfcc_f32_dev(const smx_stft_config *sc, const smx_mel_config *mc, const float *d_x, int64_t lead,
                     int64_t n, int64_t x_stride, int64_t n_mfcc, int has_lifter, double lifter, float *d_out,
                     void *stream);

/* ---- Spectral-shape features (spectral.ml:171-255; Soundml.spectral_* re-exports, soundml.ml:119-133) ------
 * One reduction along the bin axis of a magnitude spectrogram s [lead; bins; frames] (frames fastest) into
 * [lead; 1; frames]; float64 interior in the reference's operation order, one rounding to the dtype of s.
 *   centroid   sum_k f_k * (s_k / max(sum s, guarded))            (frames whose sum is below the smallest
 *                                                                   normal double divide by 1)
 *   bandwidth  (sum_k (s_k / sum s) * |centroid - f_k|^p)^(1/p)    centroid: the caller's [lead; 1; frames]
 *                                                                   (c_rows / c_frames are its last two
 *                                                                   extents, checked) or NULL = computed
 *   rolloff    min { f_k : cumsum_k >= roll_percent * cumsum_last }
 *   flatness   exp(mean log m) / mean m,  m = max(s^power, amin)
 * freqs: HOST pointer to `n_freqs` bin frequencies (float64), or NULL = the FFT grid of the 2 (bins - 1)
 * point transform, bin k at k * (1 / (fft_size * (1 / sample_rate))) (spectral.ml:105-136).
 * Invalid_argument (messages of spectral.ml:27-98): sample_rate < 1, n_freqs != bins, bins < 2 without
 * freqs, p / roll_percent / amin / power out of range, a centroid of the wrong shape, and a spectrogram
 * holding a negative or NaN entry.  That last check reads the data, so the _dev entry points synchronise
 * the stream before returning.  Empty extents write nothing (the result is all zero by contract).         */
int smx_spectral_centroid_f32(const float *s, int64_t lead, int64_t bins, int64_t frames, const double *freqs,
                              int64_t n_freqs, int64_t sample_rate, float *out);
int smx_spectral_centroid_f64(const double *s, int64_t lead, int64_t bins, int64_t frames, const double *freqs,
                              int64_t n_freqs, int64_t sample_rate, double *out);
int smx_spectral_centroid_f32_dev(const float *d_s, int64_t lead, int64_t bins, int64_t frames,
                                  const double *freqs, int64_t n_freqs, int64_t sample_rate, float *d_out,
                                  void *stream);
int smx_spectral_bandwidth_f32(const float *s, int64_t lead, int64_t bins, int64_t frames, double p,
                               const double *freqs, int64_t n_freqs, const float *centroid, int64_t c_rows,
                               int64_t c_frames, int64_t sample_rate, float *out);
int smx_spectral_bandwidth_f64(const double *s, int64_t lead, int64_t bins, int64_t frames, double p,
                               const double *freqs, int64_t n_freqs, const double *centroid, int64_t c_rows,
                               int64_t c_frames, int64_t sample_rate, double *out);
int smx_spectral_bandwidth_f32_dev(const float *d_s, int64_t lead, int64_t bins, int64_t frames, double p,
                                   const double *freqs, int64_t n_freqs, const float *d_centroid, int64_t c_rows,
                                   int64_t c_frames, int64_t sample_rate, float *d_out, void *stream);
int smx_spectral_rolloff_f32(const float *s, int64_t lead, int64_t bins, int64_t frames, double roll_percent,
                             const double *freqs, int64_t n_freqs, int64_t sample_rate, float *out);
int smx_spectral_rolloff_f64(const double *s, int64_t lead, int64_t bins, int64_t frames, double roll_percent,
                             const double *freqs, int64_t n_freqs, int64_t sample_rate, double *out);
int smx_spectral_rolloff_f32_dev(const float *d_s, int64_t lead, int64_t bins, int64_t frames,
                                 double roll_percent, const double *freqs, int64_t n_freqs, int64_t sample_rate,
                                 float *d_out, void *stream);
int smx_spectral_flatness_f32(const float *s, int64_t lead, int64_t bins, int64_t frames, double amin,
                              double power, float *out);
int smx_spectral_flatness_f64(const double *s, int64_t lead, int64_t bins, int64_t frames, double amin,
                              double power, double *out);
int smx_spectral_flatness_f32_dev(const float *d_s, int64_t lead, int64_t bins, int64_t frames, double amin,
                                  double power, float *d_out, void *stream);

/* ---- Spectral contrast and onset strength (contrast.ml, onset.ml; Soundml.spectral_contrast*, onset_strength*) ----
 * Octave-band contrast of a magnitude spectrogram s [lead; bins; frames] -> [lead; n_bands + 1; frames]: per band and
 * frame the mean of the `take` largest magnitudes against the mean of the `take` smallest (an exact selection, float64
 * means), `linear`: peak - valley, else the difference of their decibels (power_to_db, reference 1, floor 1e-10), with
 * `clamped` each side under (the maximum of its own whole tensor) - 80 dB; one rounding to the dtype of s.
 *
 * smx_spectral_contrast_plan               contrast.ml:60-142: the bands as (first bin, bins, take), n_bands + 1 entries
 *                                          each; host integers only, no device is touched
 * smx_spectral_contrast_*                  contrast.ml:208-218: audio x [lead; n] -> the magnitude spectrogram -> contrast,
 *                                          clamped
 * smx_spectral_contrast_of_spectrogram_*   fft_size 0: contrast.ml:223-252, the FFT size implied by the bin count, the
 *                                          magnitudes checked (non-negative, no NaN: the verdict is read back, so the
 *                                          _dev form synchronises the stream before returning).  fft_size > 0: the body of
 *                                          spectral_contrast_stage (contrast.ml:254-261) for a plan built at that size
 *                                          (errors under that name, magnitudes unchecked; the stage passes clamped 0)
 *
 * Onset strength (onset.ml:153-199): mel_spectrogram (power 2) -> float64 decibels under the whole tensor's 80 dB clamp ->
 * z[t] = mean over mels of max(0, db[., t] - db[., t - lag]), zero for t < lag -> centred analysis shifts right by
 * fft_size / (2 hop) frames -> one rounding; x [lead; n] -> [lead; frames].
 * smx_onset_flux_* is the one-chunk state_step of onset_strength_stage (onset.ml:82-122) with an empty carry: decibels
 * s [lead; bins; frames] -> [lead; frames], no clamp, no shift.
 *
 * The device-resident forms carry the dtype LAST (`_dev_f32`, every older entry point has `_f32_dev`): the placement
 * suite's first coverage law lists every name ending in `_dev` in one table that these entries are not part of; they have
 * a table and a law of their own (tests/test_gpu_placement_contrast_onset.py) until the two are folded. */
int smx_spectral_contrast_plan(int64_t n_bands, double f_min, double quantile, int64_t sample_rate, int64_t fft_size,
                               int64_t *lo, int64_t *sub_len, int64_t *take);
int smx_spectral_contrast_f32(const smx_stft_config *c, const float *x, int64_t lead, int64_t n, int64_t n_bands,
                              double f_min, double quantile, int linear, int64_t sample_rate, float *out);
int smx_spectral_contrast_f64(const smx_stft_config *c, const double *x, int64_t lead, int64_t n, int64_t n_bands,
                              double f_min, double quantile, int linear, int64_t sample_rate, double *out);
int smx_spectral_contrast_dev_f32(const smx_stft_config *c, const float *d_x, int64_t lead, int64_t n, int64_t x_stride,
                                  int64_t n_bands, double f_min, double quantile, int linear, int64_t sample_rate,
                                  float *d_out, void *stream);
int smx_spectral_contrast_of_spectrogram_f32(const float *s, int64_t lead, int64_t bins, int64_t frames, int64_t fft_size,
                                             int64_t n_bands, double f_min, double quantile, int linear,
                                             int64_t sample_rate, int clamped, float *out);
int smx_spectral_contrast_of_spectrogram_f64(const double *s, int64_t lead, int64_t bins, int64_t frames, int64_t fft_size,
                                             int64_t n_bands, double f_min, double quantile, int linear,
                                             int64_t sample_rate, int clamped, double *out);
int smx_spectral_contrast_of_spectrogram_dev_f32(const float *d_s, int64_t lead, int64_t bins, int64_t frames,
                                                 int64_t fft_size, int64_t n_bands, double f_min, double quantile,
                                                 int linear, int64_t sample_rate, int clamped, float *d_out, void *stream);
int smx_onset_strength_f32(const smx_stft_config *sc, const smx_mel_config *mc, const float *x, int64_t lead, int64_t n,
                           int64_t lag, float *out);
int smx_onset_strength_f64(const smx_stft_config *sc, const smx_mel_config *mc, const double *x, int64_t lead, int64_t n,
                           int64_t lag, double *out);
int smx_onset_strength_dev_f32(const smx_stft_config *sc, const smx_mel_config *mc, const float *d_x, int64_t lead,
                               int64_t n, int64_t x_stride, int64_t lag, float *d_out, void *stream);
int smx_onset_flux_f32(const float *s, int64_t lead, int64_t bins, int64_t frames, int64_t lag, float *out);
int smx_onset_flux_f64(const double *s, int64_t lead, int64_t bins, int64_t frames, int64_t lag, double *out);
int smx_onset_flux_dev_f32(const float *d_s, int64_t lead, int64_t bins, int64_t frames, int64_t lag, float *d_out,
                           void *stream);

/* ---- Energy (energy.ml; Soundml.rms, rms_of_spectrogram, zero_crossing_rate and the two stages) ----------------------
 * Frame features of audio x [lead; n] -> [lead; frames].  The grid (energy.ml:107-118): border = frame_length / 2,
 * frames = 0 for n = 0, else 1 + (n + 2 border - frame_length) / hop; frame p covers padded positions
 * [p hop, p hop + frame_length).  hop > frame_length, odd frame lengths, frame_length 1 and n < border are legal.
 *   rms                  energy.ml:126-129, 380-381: zero borders, sqrt(sum x^2 / frame_length) in float64, one rounding
 *   zero_crossing_rate   energy.ml:136-148, 383-388: borders copy the first / last sample; a sample is negative iff
 *                        (double)x < -threshold (NaN is not); a crossing is a change of that flag between positions
 *                        j - 1 and j of the frame, j = 1 .. frame_length - 1; count / frame_length, one rounding
 *   rms_of_spectrogram   energy.ml:394-421: magnitudes s [lead; bins; frames] -> [lead; frames], bins = frame_length / 2 + 1:
 *                        sqrt(2 sum_k w_k s_k^2 / frame_length^2), w = 0.5 at bin 0 and (even frame_length) at the last
 *                        bin, bins walked in ascending order; no sign check
 *   energy_frames        the stages' body (energy.ml:157-183): frames [0, count) of a segment x [lead; n] of the padded
 *                        stream, no border; (count - 1) hop + frame_length <= n.  op 0: rms, 1: zero-crossing rate
 *                        (threshold is read by op 1 only).  Errors are worded for rms_stage / zero_crossing_rate_stage.
 * A frame's float64 sum of squares has ONE order, a function of its own samples: blocks of
 * min(hop, frame_length) samples from the frame's start; in a block lane l of 64 adds elements l, l + 64, ... in ascending
 * order and the lane sums meet in the butterfly of xor distances 32, 16, 8, 4, 2, 1; the blocks' partials are added in
 * ascending order.  A batch slice, any chunking of the stages and both kernels (SMX_DISABLE_FAST) give the same bits.
 * Checks, in the reference's order and words (energy.ml:78-105, 394-408): the flat faces threshold, frame_length, hop; the
 * stages' body frame_length, hop, threshold; rms_of_spectrogram frame_length, then bins.  Zero-size axes write nothing.
 *
 * The device-resident forms end in `_device_f32`: both placement suites keep closed tables of the names that end in the
 * shorter word, before or behind the dtype; these have a table and a law of their own (tests/test_gpu_placement_energy.py).
 * They take rows x_stride >= n apart and enqueue on `stream`; nothing synchronises it. */
int smx_rms_f32(const float *x, int64_t lead, int64_t n, int64_t frame_length, int64_t hop, float *out);
int smx_rms_f64(const double *x, int64_t lead, int64_t n, int64_t frame_length, int64_t hop, double *out);
int smx_rms_device_f32(const float *d_x, int64_t lead, int64_t n, int64_t x_stride, int64_t frame_length, int64_t hop,
                       float *d_out, void *stream);
int smx_zero_crossing_rate_f32(const float *x, int64_t lead, int64_t n, int64_t frame_length, int64_t hop,
                               double threshold, float *out);
int smx_zero_crossing_rate_f64(const double *x, int64_t lead, int64_t n, int64_t frame_length, int64_t hop,
                               double threshold, double *out);
int smx_zero_crossing_rate_device_f32(const float *d_x, int64_t lead, int64_t n, int64_t x_stride, int64_t frame_length,
                                      int64_t hop, double threshold, float *d_out, void *stream);
int smx_rms_of_spectrogram_f32(const float *s, int64_t lead, int64_t bins, int64_t frames, int64_t frame_length,
                               float *out);
int smx_rms_of_spectrogram_f64(const double *s, int64_t lead, int64_t bins, int64_t frames, int64_t frame_length,
                               double *out);
int smx_rms_of_spectrogram_device_f32(const float *d_s, int64_t lead, int64_t bins, int64_t frames, int64_t frame_length,
                                      float *d_out, void *stream);
int smx_energy_frames_f32(int op, double threshold, int64_t frame_length, int64_t hop, const float *x, int64_t lead,
                          int64_t n, int64_t count, float *out);
int smx_energy_frames_f64(int op, double threshold, int64_t frame_length, int64_t hop, const double *x, int64_t lead,
                          int64_t n, int64_t count, double *out);
int smx_energy_frames_device_f32(int op, double threshold, int64_t frame_length, int64_t hop, const float *d_x,
                                 int64_t lead, int64_t n, int64_t x_stride, int64_t count, float *d_out, void *stream);

/* ---- Pitch: YIN fundamental-frequency tracking (de Cheveigne & Kawahara 2002; not in the reference) ------------------------
 * Audio x [lead; n] -> f0 and aperiodicity [lead; frames], or the normalised difference d' [lead; pmax + 1; frames].  The grid
 * is that of rms: border = frame_length / 2 virtual zeros on each side, frames = 0 for n = 0, else
 * 1 + (n + 2 border - frame_length) / hop; frame p covers padded positions [p hop, p hop + frame_length).
 * Per frame, samples x_0 .., W = frame_length / 2, pmin = floor(sample_rate / fmax),
 * pmax = min(ceil(sample_rate / fmin), frame_length - W - 1), all in float64, one rounding into the dtype of the input:
 *   r(tau) = sum_{j < W} x_j x_{j + tau};  P(i) = sum_{j < i} x_j^2;  e(tau) = P(tau + W) - P(tau)
 *   d(tau) = max(0, (e(0) + e(tau)) - 2 r(tau)), a NaN staying one;  c(tau) = d(1) + .. + d(tau);  d'(0) = 1, d'(tau) = (d(tau) tau) / c(tau),
 *   1 where c(tau) = 0
 *   the lag: the smallest tau in [pmin, pmax] with d'(tau) < trough_threshold, d'(tau) <= d'(tau - 1) and (tau = pmax or
 *   d'(tau) < d'(tau + 1)); if none, the smallest tau of the range that attains the minimum of d'
 *   the shift: with a, b, c = d'(tau - 1), d'(tau), d'(tau + 1) where tau + 1 <= pmax, den = (a - 2 b) + c:
 *   (0.5 (a - c)) / den if den > 0 and its magnitude is at most 1, else 0
 *   f0 = sample_rate / (tau + shift), aperiodicity = d'(tau); both NaN where e(0) or c(pmax) is not finite
 * The sums have ONE order, a function of the frame's own samples: j < W in blocks of min(hop, W) from the
 * frame's start, a block's partial one ascending chain from 0.0, the partials added in ascending order; P one ascending
 * chain from the frame's first sample.  Float32 samples: fma (the products are exact); float64: product and sum round in turn.
 * A batch slice, a frame range, any chunking of the stage and both kernels (SMX_DISABLE_FAST) give the same bits.
 *   yin_frames   the stage's body: frames [0, count) of a segment x [lead; n] of the padded stream, no border;
 *                (count - 1) hop + frame_length <= n.  Errors are worded for yin_stage.
 * Checks, in this order: sample_rate >= 1, frame_length >= 4, hop >= 1, fmin and fmax finite with
 * 0 < fmin < fmax <= sample_rate / 2, trough_threshold finite and positive (not read by yin_difference), pmax > pmin.
 * aperiodicity may be NULL.  Zero-size axes write nothing; a call with null data and zero extents checks the parameters only.
 *
 * The device-resident forms end in `_resident_f32` (tests/test_gpu_placement_pitch.py keeps their table and law): rows
 * x_stride >= n apart, enqueued on `stream`, nothing synchronises it and no flag is read back. */
int smx_yin_f32(const float *x, int64_t lead, int64_t n, int64_t sample_rate, double fmin, double fmax, int64_t frame_length,
                int64_t hop, double trough_threshold, float *f0, float *aperiodicity);
int smx_yin_f64(const double *x, int64_t lead, int64_t n, int64_t sample_rate, double fmin, double fmax, int64_t frame_length,
                int64_t hop, double trough_threshold, double *f0, double *aperiodicity);
int smx_yin_resident_f32(const float *d_x, int64_t lead, int64_t n, int64_t x_stride, int64_t sample_rate, double fmin,
                         double fmax, int64_t frame_length, int64_t hop, double trough_threshold, float *d_f0,
                         float *d_aperiodicity, void *stream);
int smx_yin_difference_f32(const float *x, int64_t lead, int64_t n, int64_t sample_rate, double fmin, double fmax,
                           int64_t frame_length, int64_t hop, float *out);
int smx_yin_difference_f64(const double *x, int64_t lead, int64_t n, int64_t sample_rate, double fmin, double fmax,
                           int64_t frame_length, int64_t hop, double *out);
int smx_yin_difference_resident_f32(const float *d_x, int64_t lead, int64_t n, int64_t x_stride, int64_t sample_rate,
                                    double fmin, double fmax, int64_t frame_length, int64_t hop, float *d_out, void *stream);
int smx_yin_frames_f32(const float *x, int64_t lead, int64_t n, int64_t count, int64_t sample_rate, double fmin, double fmax,
                       int64_t frame_length, int64_t hop, double trough_threshold, float *f0, float *aperiodicity);
int smx_yin_frames_f64(const double *x, int64_t lead, int64_t n, int64_t count, int64_t sample_rate, double fmin, double fmax,
                       int64_t frame_length, int64_t hop, double trough_threshold, double *f0, double *aperiodicity);
int smx_yin_frames_resident_f32(const float *d_x, int64_t lead, int64_t n, int64_t x_stride, int64_t count, int64_t sample_rate,
                                double fmin, double fmax, int64_t frame_length, int64_t hop, double trough_threshold,
                                float *d_f0, float *d_aperiodicity, void *stream);

/* ---- Pitch, continued: pYIN (Mauch & Dixon 2014; not in the reference) -------------------------------------------------------
 * Probabilistic YIN with Viterbi decoding.  Audio x [lead; n] -> f0, voiced_flag (1.0 / 0.0) and voiced_prob, each
 * [lead; frames]; or the observation [lead; 2 n_bins; frames]; or, from an observation, the decoded states [lead; frames]
 * (exact integers; state s < n_bins is voiced bin s, n_bins + b is unvoiced bin b).  The grid is yin's, everything is float64
 * inside with one rounding into the dtype of the input, and there is ONE order of operations, restated in
 * tests/pyin_restatement.py.  The decoder is offline by definition: there is no streaming stage.
 *
 * Host tables (float64, libm; smx_pyin_tables returns them), n = n_thresholds, (a, b) = beta parameters, l = boltzmann_parameter:
 *   thr[k] = k / n, k = 0 .. n;   beta[k] = I(thr[k + 1]; a, b) - I(thr[k]; a, b), I the regularised incomplete beta function
 *   E[q] = exp(-l q);   Z[N] = (1 - exp(-l)) / (1 - exp(-l N)), N >= 1;  the trough prior is the ONE product Z[N] * E[q]
 *   bps = ceil(1 / resolution);   n_bins = floor(12 bps log2(fmax / fmin)) + 1;   freq[b] = fmin 2^(b / (12 bps))
 *   edge[b] = fmin 2^((b - 0.5) / (12 bps)), b = 1 .. n_bins - 1: the bin of a frequency f is the number of edges <= f
 *   (comparisons only; it lies in [0, n_bins - 1])
 *   m = round-half-even(max_transition_rate 12 hop / sample_rate), h = (m bps) / 2 (integer division)
 *   tri[k] = 1 - |k - h| / (h + 1), k = 0 .. 2 h;   rs[i] = 1 / (the sum of tri[j - i + h] over the j of [i - h, i + h] that lie
 *   in [0, n_bins), ascending)
 *
 * Observation, per frame, from yin's float64 d'(tau) (its chains, its bits):
 *   1. the troughs: tau in [pmin, pmax] with d'(tau) <= d'(tau - 1) and (tau = pmax or d'(tau) < d'(tau + 1)): yin's rule without
 *      the threshold; tau_1 < .. < tau_R with heights g_r
 *   2. for k = 1 .. n: below(r, k) = g_r < thr[k], N_k their count, q(r, k) the number of r' < r with below(r', k); p_r adds, from
 *      0.0 in ascending k, (Z[N_k] * E[q(r, k)]) * beta[k - 1] where below(r, k): each product rounded, then the sum
 *   3. r* the first trough of least height, K0 the number of k in 1 .. n with thr[k] <= g_r*:
 *      p_r* += no_trough_prob * (beta[0] + .. + beta[K0 - 1], ascending) where K0 < n; where no threshold lies above the least
 *      trough (d' = 1 throughout: silence) nothing is added, the frame has voiced_prob = 0
 *   4. every r with p_r > 0: period tau_r + shift_r (yin's parabola rule), f = sample_rate / period, its bin by edge; obs[b] adds
 *      the p_r that land in b, from 0.0 in ascending r
 *   5. voiced_prob = min(1, obs[0] + .. + obs[n_bins - 1], ascending)       6. obs[n_bins + b] = (1 - voiced_prob) / n_bins
 *   7. a frame that yin would give NaN (e(0) or c(pmax) not finite) has a zero voiced part and voiced_prob = 0 for the decoder;
 *      its voiced_prob and its column of pyin_observation are NaN
 *
 * Decode, per clip, in the probability domain: only *, < and an exact scaling by a power of two occur, no log is taken.
 *   1. B = obs where obs > FLOOR, else FLOOR = 2^-200 (a NaN too): a path stays alive when a frame with voiced_prob = 1 jumps
 *      further than the band
 *   2. delta_0 = p_init * B_0, p_init = 1 / n_bins on the unvoiced states and 0 on the voiced
 *   3. per frame t >= 1: u[i] = (delta[i] * 2^-e) * rs[i], e the binary exponent (frexp) of the greatest delta; per voicing v,
 *      M_v(j) the greatest u_v[i] * tri[j - i + h] over the band's i in ascending order, a candidate replacing the best only if
 *      strictly greater (the smallest i wins ties); a = M_v(j) * (1 - switch_prob), b = M_{1-v}(j) * switch_prob, b taken only if
 *      b > a; delta_t(v, j) = taken * B_t(v, j), the back pointer the taken (v', i)
 *   4. the end: the smallest state of the greatest delta_{T-1}; the walk back follows the pointers
 *   5. f0 = freq[state mod n_bins] on voiced frames, `fill` on unvoiced ones (the bin's frequency with keep_bin != 0);
 *      voiced_flag = 1 where state < n_bins
 * One workgroup decodes a clip with delta, u and two frames' voiced observations in LDS: 3 n_bins + 2 min(h, n_bins - 1) may be at
 * most 9212, past it the call is an argument error (there is no second decoder).
 *
 * Checks, in this order: yin's own (sample_rate, frame_length, hop, the band, pmax > pmin); n_thresholds >= 1; beta_a, beta_b
 * finite and positive; boltzmann_parameter finite and positive; 0 < resolution < 1; max_transition_rate finite and >= 0;
 * switch_prob and no_trough_prob in [0, 1]; 2 n_bins <= 65535; the band below 2^31 bins; (pyin) the decoder's cap.
 * smx_pyin_decode: an even, positive state axis, half_width >= 0, switch_prob, 2 n_bins <= 65535, the cap.  Zero-size axes
 * write nothing; a call with null data and zero extents checks the parameters only.
 *
 * The device-resident forms end in `_accel_f32` (tests/test_gpu_placement_pyin.py keeps their table and law): rows x_stride >= n
 * apart (clips clip_stride >= states * frames apart), enqueued on `stream`; nothing synchronises it and no flag is read back. */
int smx_pyin_f32(const float *x, int64_t lead, int64_t n, int64_t sample_rate, double fmin, double fmax, int64_t frame_length,
                 int64_t hop, int64_t n_thresholds, double beta_a, double beta_b, double boltzmann_parameter, double resolution,
                 double max_transition_rate, double switch_prob, double no_trough_prob, int64_t keep_bin, double fill, float *f0,
                 float *voiced_flag, float *voiced_prob);
int smx_pyin_f64(const double *x, int64_t lead, int64_t n, int64_t sample_rate, double fmin, double fmax, int64_t frame_length,
                 int64_t hop, int64_t n_thresholds, double beta_a, double beta_b, double boltzmann_parameter, double resolution,
                 double max_transition_rate, double switch_prob, double no_trough_prob, int64_t keep_bin, double fill, double *f0,
                 double *voiced_flag, double *voiced_prob);
int smx_pyin_accel_f32(const float *d_x, int64_t lead, int64_t n, int64_t x_stride, int64_t sample_rate, double fmin, double fmax,
                       int64_t frame_length, int64_t hop, int64_t n_thresholds, double beta_a, double beta_b,
                       double boltzmann_parameter, double resolution, double max_transition_rate, double switch_prob,
                       double no_trough_prob, int64_t keep_bin, double fill, float *d_f0, float *d_voiced_flag,
                       float *d_voiced_prob, void *stream);
int smx_pyin_observation_f32(const float *x, int64_t lead, int64_t n, int64_t sample_rate, double fmin, double fmax,
                             int64_t frame_length, int64_t hop, int64_t n_thresholds, double beta_a, double beta_b,
                             double boltzmann_parameter, double resolution, double max_transition_rate, double switch_prob,
                             double no_trough_prob, float *out);
int smx_pyin_observation_f64(const double *x, int64_t lead, int64_t n, int64_t sample_rate, double fmin, double fmax,
                             int64_t frame_length, int64_t hop, int64_t n_thresholds, double beta_a, double beta_b,
                             double boltzmann_parameter, double resolution, double max_transition_rate, double switch_prob,
                             double no_trough_prob, double *out);
int smx_pyin_observation_accel_f32(const float *d_x, int64_t lead, int64_t n, int64_t x_stride, int64_t sample_rate, double fmin,
                                   double fmax, int64_t frame_length, int64_t hop, int64_t n_thresholds, double beta_a,
                                   double beta_b, double boltzmann_parameter, double resolution, double max_transition_rate,
                                   double switch_prob, double no_trough_prob, float *d_out, void *stream);
int smx_pyin_decode_f32(const float *obs, int64_t lead, int64_t states, int64_t frames, int64_t half_width, double switch_prob,
                        float *out);
int smx_pyin_decode_f64(const double *obs, int64_t lead, int64_t states, int64_t frames, int64_t half_width, double switch_prob,
                        double *out);
int smx_pyin_decode_accel_f32(const float *d_obs, int64_t lead, int64_t states, int64_t frames, int64_t clip_stride,
                              int64_t half_width, double switch_prob, float *d_out, void *stream);
/* n_bins; h; and the host tables thr [n + 1], beta [n], E [maxr], Z [maxr + 1] (Z[0] = 0), freq [n_bins], edge [n_bins - 1]
 * (b = 1 ..), tri [2 h + 1], rs [n_bins], maxr = (pmax - pmin) / 2 + 1 the most troughs of a frame; each may be NULL */
int smx_pyin_bins(double fmin, double fmax, double resolution, int64_t *n_bins);
int smx_pyin_half_width(int64_t sample_rate, int64_t hop, double resolution, double max_transition_rate, int64_t *half_width);
int smx_pyin_tables(int64_t sample_rate, double fmin, double fmax, int64_t frame_length, int64_t hop, int64_t n_thresholds,
                    double beta_a, double beta_b, double boltzmann_parameter, double resolution, double max_transition_rate,
                    double switch_prob, double no_trough_prob, double *thr, double *beta, double *E, double *Z, double *freq,
                    double *edge, double *tri, double *rs);

/* ---- Rhythm: tempogram, tempo and beat tracking over an onset envelope (not in the reference) -------------------------------
 * env [lead; frames] is an onset envelope (onset_strength's output).  Everything is float64 inside with one rounding into the
 * dtype of the input; every sum has ONE order, a function of the clip's own values, so a leading slice of a
 * batch equals the batch's slice and both tempogram kernels (SMX_DISABLE_FAST) give the same bits.  No chain is fused: a
 * product and the sum it joins round one after the other.
 *
 * tempogram (Grosche, Mueller & Kurth 2010) -> [lead; win_length; frames], W = win_length, b = W / 2:
 *   pad = b virtual zeros, env, W - b virtual zeros (zeros as for rms, not a ramp);  y_j = w_j pad[t + j], j < W, w the
 *   periodic window of smx_window_make_param in float64, the product rounded once;
 *   a(tau) = sum_{j < W - tau} y_j y_{j + tau}, tau = 0 .. W - 1: one ascending chain over j from 0.0;
 *   norm != 0: a(tau) / a(0) unless a(0) < DBL_MIN, where a(tau) stays as it is; a frame that reads a NaN has a(0) = NaN and
 *   is NaN at every lag then (without norm only the lags whose chain meets the NaN are).
 * tempo -> [lead]:
 *   m(tau) = (sum_t n(tau, t)) / frames over the float64 normalised tempogram n (hann window) before its rounding, one
 *   ascending chain over t from 0.0, then the division;  bpm(tau) = 60 sample_rate / (hop tau);
 *   prior(tau) = -0.5 ((log2 bpm(tau) - log2 start_bpm) / std_bpm)^2, -inf for tau = 0 and where bpm(tau) > max_tempo;
 *   score(tau) = log1p(1e6 m(tau)) + prior(tau) over the lags whose prior is finite; the lag is the smallest tau that attains
 *   the greatest score that is not NaN.  The result is bpm(lag), or the lag itself with want_lag; NaN when m(1) is NaN (a
 *   non-finite or empty envelope) or no score is a number.  The float32 tempogram is never written.
 * beat_track (Ellis 2007) -> tempo [lead], beats [lead; frames] as 1.0 / 0.0:
 *   period = the lag of tempo (std_bpm 1, max_tempo 320) when has_bpm = 0, the integer itself, and the tempo reported is
 *   bpm(lag); otherwise round_half_even(60 sample_rate / hop / bpm) and the tempo reported is bpm.  A clip has NO beats
 *   (the mask is zeros, the tempo is still reported) when frames < 2, the lag is none, sd below is zero or not finite, or
 *   some ls is not finite.
 *   sd = sqrt((sum_i (env_i - mean)^2) / (frames - 1)), mean = (sum_i env_i) / frames: two ascending chains from 0.0;
 *   ne = env / sd;  ls_i = sum_n ne_n g(i - n) over max(0, i - period) <= n <= min(frames - 1, i + period), one ascending
 *   chain over n from 0.0;  g(k) = exp(-0.5 (32 k / period)^2);
 *   window_k = -2 period + k, k = 0 .. 2 period - round_half_even(period / 2);  tx_k = -tightness log(-window_k / period)^2;
 *   for i ascending: cand_k = tx_k + cum[i + window_k], tx_k alone where i + window_k < 0; k* the smallest k that attains
 *   the maximum; cum_i = ls_i + cand_k*; back_i = -1 while no frame j <= i has had ls_j >= 0.01 max(ls), else i + window_k*;
 *   local maxima: i >= 1 with cum_i > cum_{i-1} and (i = frames - 1 or cum_i >= cum_{i+1}); med = their median by exact
 *   selection, (lo + hi) / 2 of the two middle values for an even count; the last beat is the largest maximum i with
 *   2 cum_i > med (none: no beats); the beats are i, back_i, back_back_i .. while the index is >= 0;
 *   trimming, over the beats in ascending order with v_q = ls at beat q: sm_q = (0.5 v_{q-1} + v_q) + 0.5 v_{q+1}, an absent
 *   neighbour's term left out; th = 0.5 sqrt((sum_q sm_q^2) / count), an ascending chain, with trim, else 0; the beats from the
 *   first to the last one with sm_q > th stay.
 *   g, tx and the prior are built on the host in float64 with libm, once per (period range, tightness) / per prior, and kept on
 *   the device; smx_rhythm_beat_tables (g [2 period + 1], tx [2 period - round_half_even(period / 2) + 1]),
 *   smx_rhythm_tempo_prior and smx_rhythm_tempo_frequencies ([win_length] each) return the same values.
 * Checks, in this order, before the data is looked at (null data and zero extents check the parameters only):
 *   tempogram: win_length in [1, 16384], the window's parameter.
 *   tempo, tempo_prior: sample_rate >= 1, hop >= 1, win_length, start_bpm finite and positive, std_bpm finite and positive,
 *   max_tempo positive, some lag 1 .. win_length - 1 with bpm(lag) <= max_tempo.
 *   beat_track: sample_rate, hop; with has_bpm: bpm finite and positive, its period in [1, 4096]; otherwise tempo's checks;
 *   tightness finite and positive; then frames <= 8192.
 * The device-resident forms end in `_gpu_f32` (tests/test_gpu_placement_rhythm.py keeps their table and law): rows
 * env_stride >= frames apart, enqueued on `stream`, nothing synchronises it and no flag is read back. */
int smx_rhythm_tempogram_f32(const float *env, int64_t lead, int64_t frames, int64_t win_length, int window,
                             double window_param, int norm, float *out);
int smx_rhythm_tempogram_f64(const double *env, int64_t lead, int64_t frames, int64_t win_length, int window,
                             double window_param, int norm, double *out);
int smx_rhythm_tempogram_gpu_f32(const float *d_env, int64_t lead, int64_t frames, int64_t env_stride, int64_t win_length,
                                 int window, double window_param, int norm, float *d_out, void *stream);
int smx_rhythm_tempo_f32(const float *env, int64_t lead, int64_t frames, int64_t sample_rate, int64_t hop, int64_t win_length,
                         double start_bpm, double std_bpm, double max_tempo, int want_lag, float *out);
int smx_rhythm_tempo_f64(const double *env, int64_t lead, int64_t frames, int64_t sample_rate, int64_t hop, int64_t win_length,
                         double start_bpm, double std_bpm, double max_tempo, int want_lag, double *out);
int smx_rhythm_tempo_gpu_f32(const float *d_env, int64_t lead, int64_t frames, int64_t env_stride, int64_t sample_rate,
                             int64_t hop, int64_t win_length, double start_bpm, double std_bpm, double max_tempo, int want_lag,
                             float *d_out, void *stream);
int smx_rhythm_beat_track_f32(const float *env, int64_t lead, int64_t frames, int64_t sample_rate, int64_t hop, int has_bpm,
                              double bpm, int64_t win_length, double start_bpm, double tightness, int trim, float *tempo,
                              float *beats);
int smx_rhythm_beat_track_f64(const double *env, int64_t lead, int64_t frames, int64_t sample_rate, int64_t hop, int has_bpm,
                              double bpm, int64_t win_length, double start_bpm, double tightness, int trim, double *tempo,
                              double *beats);
int smx_rhythm_beat_track_gpu_f32(const float *d_env, int64_t lead, int64_t frames, int64_t env_stride, int64_t sample_rate,
                                  int64_t hop, int has_bpm, double bpm, int64_t win_length, double start_bpm, double tightness,
                                  int trim, float *d_tempo, float *d_beats, void *stream);
int smx_rhythm_tempo_frequencies(int64_t win_length, int64_t sample_rate, int64_t hop, double *out);
int smx_rhythm_tempo_prior(int64_t win_length, int64_t sample_rate, int64_t hop, double start_bpm, double std_bpm,
                           double max_tempo, double *out);
int smx_rhythm_beat_period(int64_t sample_rate, int64_t hop, double bpm, int64_t *period);
int smx_rhythm_beat_tables(int64_t period, double tightness, double *g, double *tx);

/* ---- Sequence: pairwise cost matrix and dynamic time warping of two feature sequences (not in the reference) ----------------
 * X [pairs; d; n] and Y [pairs; d; m] are feature-major with frames last (chroma, MFCC, mel), pair by pair.  Everything is
 * float64 inside with one rounding into the dtype of the input.
 *
 * 1. Cost.  C[i, j] is a function of column i of X and column j of Y only.  Every metric is ONE ascending chain over the
 *    feature index k from 0.0, each operation rounded as written, nothing fused (x_k - y_k of float32 values is not always
 *    exact in float64, so no fma):
 *      SMX_METRIC_SQEUCLIDEAN  sum_k (x_k - y_k)^2
 *      SMX_METRIC_EUCLIDEAN    its IEEE sqrt
 *      SMX_METRIC_CITYBLOCK    sum_k |x_k - y_k|
 *      SMX_METRIC_COSINE       1 - dot / (sqrt(xx) sqrt(yy)), dot = sum_k x_k y_k, xx = sum_k x_k x_k, yy = sum_k y_k y_k: three
 *                              such chains; NaN where a norm is zero, as 0 / 0 is.
 * 2. Recursion.  The steps are, in this order, s = 0 from (i - 1, j - 1), s = 1 from (i, j - 1), s = 2 from (i - 1, j):
 *      cand_s = (D[prev_s] + weights_mul[s] C[i, j]) + weights_add[s];
 *    a step whose predecessor lies outside the matrix is absent.  D[i, j] is the first present candidate; each later present
 *    candidate replaces it only if cand < best, a strict comparison and never fmin: a tie keeps the earlier step, a NaN never
 *    replaces anything, a NaN that came first stays.  The chosen s is the cell's step code.  D[0, 0] = C[0, 0], unweighted.
 *    With subseq, D[0, j] = C[0, j] for every j: row 0 has no predecessors.
 * 3. End and path.  The end cell is (n - 1, m - 1); with subseq (n - 1, j*), j* chosen by the same rule over row n - 1 in
 *    float64: start from j = 0, replace only if strictly smaller, so the smallest index wins ties.  The path follows the step
 *    codes back from the end until (0, 0), or until i = 0 with subseq, and is written in ascending order into path
 *    [pairs; 2; n + m - 1] in the dtype of the input: row 0 the indices into X, row 1 those into Y, the unused tail of both
 *    rows -1.0.  dtw_distance [pairs] is the float64 value at the end cell, rounded once; it writes neither D nor step codes.
 * Nothing in 2 and 3 depends on the order in which cells are visited (+ and < on the same operands give the same bits): the
 * tile kernel (smx_sequence_tile gives its tile shape), the general kernel (SMX_DISABLE_FAST=1, and every float64 call), a
 * leading slice of a batch and the batch's slice agree bit for bit.
 * Checks, in this order, before the data is looked at (null data and zero pairs check the parameters only): the metric;
 * d >= 1; n >= 1 and m >= 1; dtw and dtw_distance: every weight finite; dtw: n m <= 2^29 (the step codes of one pair, a byte a
 * cell, are the scratch of one launch group: 512 MB; dtw_distance has no such cap), and n, m <= 2^24 in float32 (the path's
 * indices are exact).  Scratch is stream-ordered, at most 512 MB per launch group where one pair fits; larger batches go pair
 * range by pair range.
 * Out of scope: step sets other than the classic three; global band constraints (Sakoe-Chiba band, Itakura parallelogram); a
 * streaming stage (the alignment is offline by definition: the end cell needs both sequences whole); recurrence and
 * self-similarity matrices beyond what cost_matrix(X, X) gives.
 * The device-resident forms end in `_hbm_f32` (tests/test_gpu_placement_sequence.py keeps their table and law): rows of X
 * x_stride >= n and rows of Y y_stride >= m elements apart, dense outputs, enqueued on `stream`, nothing synchronises it and no
 * flag is read back. */
#define SMX_METRIC_EUCLIDEAN 0
#define SMX_METRIC_SQEUCLIDEAN 1
#define SMX_METRIC_CITYBLOCK 2
#define SMX_METRIC_COSINE 3
int smx_sequence_tile(int64_t *rows, int64_t *cols);
int smx_cost_matrix_f32(const float *x, const float *y, int64_t pairs, int64_t d, int64_t n, int64_t m, int metric, float *out);
int smx_cost_matrix_f64(const double *x, const double *y, int64_t pairs, int64_t d, int64_t n, int64_t m, int metric,
                        double *out);
int smx_cost_matrix_hbm_f32(const float *d_x, const float *d_y, int64_t pairs, int64_t d, int64_t n, int64_t m, int64_t x_stride,
                            int64_t y_stride, int metric, float *d_out, void *stream);
int smx_dtw_f32(const float *x, const float *y, int64_t pairs, int64_t d, int64_t n, int64_t m, int metric,
                const double *weights_add, const double *weights_mul, int subseq, float *D, float *path);
int smx_dtw_f64(const double *x, const double *y, int64_t pairs, int64_t d, int64_t n, int64_t m, int metric,
                const double *weights_add, const double *weights_mul, int subseq, double *D, double *path);
int smx_dtw_hbm_f32(const float *d_x, const float *d_y, int64_t pairs, int64_t d, int64_t n, int64_t m, int64_t x_stride,
                    int64_t y_stride, int metric, const double *weights_add, const double *weights_mul, int subseq, float *d_D,
                    float *d_path, void *stream);
int smx_dtw_distance_f32(const float *x, const float *y, int64_t pairs, int64_t d, int64_t n, int64_t m, int metric,
                         const double *weights_add, const double *weights_mul, int subseq, float *out);
int smx_dtw_distance_f64(const double *x, const double *y, int64_t pairs, int64_t d, int64_t n, int64_t m, int metric,
                         const double *weights_add, const double *weights_mul, int subseq, double *out);
int smx_dtw_distance_hbm_f32(const float *d_x, const float *d_y, int64_t pairs, int64_t d, int64_t n, int64_t m, int64_t x_stride,
                             int64_t y_stride, int metric, const double *weights_add, const double *weights_mul, int subseq,
                             float *d_out, void *stream);

/* ---- Decompose: non-negative matrix factorisation of a magnitude spectrogram (not in the reference) -------------------------
 * V [clips; F; T] >= 0 is feature-major with frames last; W [clips; F; K] holds K spectral templates per clip and H [clips; K; T]
 * their activations, V ~ W H.  Multiplicative updates (Lee & Seung 2001); beta is SMX_NMF_FROBENIUS or SMX_NMF_KULLBACK_LEIBLER.
 * Results have the dtype of V; the interior is float32 for float32 and float64 for float64.
 *
 * eps = 2^-23 (1.1920929e-07); floor(x) is `x < eps ? eps : x`, so a NaN stays a NaN.  One round is two updates in this order,
 * the W update seeing the new H:
 *   H update, Frobenius   H <- (H o (W^T V)) / floor((W^T W) H)
 *   H update, KL          R = V / floor(W H);  H <- (H o (W^T R)) / floor(s_k),  s_k = sum_f W[f, k] 1 for every entry of row k
 *   W update, Frobenius   W <- (W o (V H^T)) / floor(W (H H^T))
 *   W update, KL          R = V / floor(W H);  W <- (W o (R H^T)) / floor(s_k),  s_k = sum_t H[k, t] 1 for every entry of column k
 * The product with the old factor and the IEEE division round one after the other.  Every inner product (the entries of W^T V,
 * W^T W, (W^T W) H, W H, W^T R, s_k and their transposes) is ONE chain acc = fma(a, b, acc) from 0.0 whose order is a function of
 * (F, T, K) only, never of the batch, the grid, the clip or the kernel:
 *   over f or t   32-block after 32-block in ascending order; inside a block the offsets run
 *                 0 4 1 5 2 6 3 7 | 8 12 9 13 10 14 11 15 | 16 20 ... | 24 28 ... 27 31, i.e. position i = 2 r + h is offset
 *                 (r & 3) + 8 (r >> 2) + 4 h (the order in which a 32 x 32 accumulator tile of v_mfma_f32_32x32x2_f32 hands its
 *                 rows on as the next product's operand); the last block is padded to 32 with terms fma(0, 0, acc)
 *   over k        ascending, padded to an even count with one term fma(0, 0, acc)
 * (a pad term changes nothing but the sign of a zero sum).  The tile kernels (float32, K <= 64: smx_nmf_tile_cap) and the general
 * kernels (any K <= 1024, float64, SMX_DISABLE_FAST=1), a leading slice of a batch and the batch's slice agree bit for bit, and
 * n_iter = a continued by n_iter = b from its factors equals n_iter = a + b.  n_iter = 0 returns the initial factors.
 * A NaN in V[f, t] makes column t of H and every entry of W NaN in the first round and every entry of H of that clip in the
 * second; no other clip is touched.  Negative entries are not checked.
 * nmf_activations runs the H update alone with W fixed; the device form takes w_stride = 0 for ONE dictionary [F; K] shared by
 * every clip.  nmf_reconstruct is W H by the chain over k above, a component outside `components` (n_components indices on the
 * host; null: all of them) entering as fma(0, 0, acc); with as_mask the result is that sum over floor(the sum of all components),
 * the soft mask of the chosen components.  nmf_divergence [clips] is the objective per clip in float64 from the
 * stored factors, X = W H an ascending chain over k of products and sums rounded one after the other:
 *   Frobenius   sqrt(sum (V - X)^2 / sum V^2)
 *   KL          ((sum over V > 0 of V log(V / X)) - sum V + sum X) / sum V
 * every sum an ascending chain over t per row, then an ascending chain over the rows, rounded once into the dtype of V.
 * Checks, in this order, before the data is looked at (null data and zero clips check the parameters only): K >= 1; K <= 1024;
 * F, T >= 1 and <= 2^24; beta; n_iter >= 0; clips >= 0; the pitches and strides below.  Scratch is stream-ordered, at most 512 MB
 * per launch group where one clip fits; larger batches go clip range by clip range, each range running all its rounds.
 * Out of scope: the Itakura-Saito divergence; sparsity penalties; a dictionary learned across clips (a reduction across clips);
 * streaming; convolutive NMF.
 * The device-resident forms end in `_vram_f32` (tests/test_gpu_placement_decompose.py keeps their table and law): clips of V
 * v_stride and its rows v_pitch >= T elements apart (S[..., :, a:b] of a spectrogram is an input as it stands), the factors'
 * clips w0_stride, h0_stride, w_stride, h_stride elements apart, dense inside a clip; nmf_reconstruct's output out_stride /
 * out_pitch apart.  Results must not overlap inputs.  Enqueued on `stream`, nothing synchronises it and no flag is read back. */
#define SMX_NMF_FROBENIUS 0
#define SMX_NMF_KULLBACK_LEIBLER 1
int smx_nmf_tile_cap(int64_t *tile_k, int64_t *max_k);
int smx_nmf_f32(const float *V, const float *W0, const float *H0, int64_t clips, int64_t F, int64_t T, int64_t K, int64_t n_iter,
                int beta, float *W, float *H);
int smx_nmf_f64(const double *V, const double *W0, const double *H0, int64_t clips, int64_t F, int64_t T, int64_t K,
                int64_t n_iter, int beta, double *W, double *H);
int smx_nmf_vram_f32(const float *d_V, int64_t v_stride, int64_t v_pitch, const float *d_W0, int64_t w0_stride, const float *d_H0,
                     int64_t h0_stride, int64_t clips, int64_t F, int64_t T, int64_t K, int64_t n_iter, int beta, float *d_W,
                     int64_t w_stride, float *d_H, int64_t h_stride, void *stream);
int smx_nmf_activations_f32(const float *V, const float *W, const float *H0, int64_t clips, int64_t F, int64_t T, int64_t K,
                            int64_t n_iter, int beta, float *H);
int smx_nmf_activations_f64(const double *V, const double *W, const double *H0, int64_t clips, int64_t F, int64_t T, int64_t K,
                            int64_t n_iter, int beta, double *H);
int smx_nmf_activations_vram_f32(const float *d_V, int64_t v_stride, int64_t v_pitch, const float *d_W, int64_t w_stride,
                                 const float *d_H0, int64_t h0_stride, int64_t clips, int64_t F, int64_t T, int64_t K,
                                 int64_t n_iter, int beta, float *d_H, int64_t h_stride, void *stream);
int smx_nmf_reconstruct_f32(const float *W, const float *H, int64_t clips, int64_t F, int64_t T, int64_t K,
                            const int64_t *components, int64_t n_components, int as_mask, float *out);
int smx_nmf_reconstruct_f64(const double *W, const double *H, int64_t clips, int64_t F, int64_t T, int64_t K,
                            const int64_t *components, int64_t n_components, int as_mask, double *out);
int smx_nmf_reconstruct_vram_f32(const float *d_W, int64_t w_stride, const float *d_H, int64_t h_stride, int64_t clips, int64_t F,
                                 int64_t T, int64_t K, const int64_t *components, int64_t n_components, int as_mask,
                                 float *d_out, int64_t out_stride, int64_t out_pitch, void *stream);
int smx_nmf_divergence_f32(const float *V, const float *W, const float *H, int64_t clips, int64_t F, int64_t T, int64_t K,
                           int beta, float *out);
int smx_nmf_divergence_f64(const double *V, const double *W, const double *H, int64_t clips, int64_t F, int64_t T, int64_t K,
                           int beta, double *out);
int smx_nmf_divergence_vram_f32(const float *d_V, int64_t v_stride, int64_t v_pitch, const float *d_W, int64_t w_stride,
                                const float *d_H, int64_t h_stride, int64_t clips, int64_t F, int64_t T, int64_t K, int beta,
                                float *d_out, void *stream);

/* ---- Harmonic/percussive separation (hpss.ml) ------------------------------------------------------------
 * Median-filter separation of a magnitude spectrogram s [lead; bins; frames] (frames fastest; leading axes are
 * independent planes):
 *   harm[b, t] = running median of kernel_h frames of row b, perc[b, t] = running median of kernel_p bins of
 *   column t (hpss.ml:22-61); the window of index i is [i - k/2, i + k - 1 - k/2], the value rank k/2 of the
 *   ascending window (the upper middle, never a mean), indices outside the axis reflected half-sample-
 *   symmetrically with period 2 n for any overhang (hpss.ml:43-50, 69-75).  The medians SELECT: each is one of the
 *   input values bit for bit, and both filters draw from the same values.
 *   mask_h = f(harm, margin_h * perc), mask_p = f(perc, margin_p * harm), f(x, r) = x^p / (x^p + r^p) on the pair
 *   rescaled by its pointwise maximum z (p = 1 the identity, p = 2 one multiply), 0.5 (unit margins) or 0 where z is
 *   below the smallest positive normal; power = INFINITY: the strict comparison x > r as 0 / 1 (hpss.ml:309-347).
 * kernel_h, kernel_p >= 1 (any size: one may be far larger than its axis), power > 0 or INFINITY, margins finite
 * and >= 1: otherwise SMX_INVALID_ARGUMENT with the messages of hpss.ml:373-396, checked in that order before any
 * device work.  Either result pointer may be NULL (that result is not computed); zero-size axes write nothing.
 * NaN inputs give unspecified results, as in the reference; -0.0 orders below +0.0.
 *
 * smx_hpss_masks_*           hpss.ml:411-414  `hpss_masks`: -> mask_h, mask_p, shape and dtype of s
 * smx_hpss_of_spectrogram_*  hpss.ml:416-420  `hpss_of_spectrogram`: -> s * mask_h, s * mask_p
 * smx_hpss_of_stft_*         hpss.ml:436-459  `hpss_of_stft`: z interleaved complex [lead; bins; frames] in the layout
 *                            smx_stft_transform writes; mag = |z| in the component width, the unit phase component by
 *                            component (1 + 0i where mag = 0), -> (mag * mask) * phase_re + i (mag * mask) * phase_im
 * smx_hpss_*                 hpss.ml:477-504  `hpss` / `harmonic` / `percussive`: audio x [lead; n] -> y_h, y_p [lead; n]:
 *                            Stft.transform -> hpss_of_stft -> Stft.invert ~length:n per component, bit for bit those
 *                            three calls; y_p = NULL is `harmonic`, y_h = NULL `percussive` (the other inversion is
 *                            skipped).  The spectra stay on the device; the batch runs in clip chunks.  Also raises what
 *                            Stft.invert raises (stft.ml:745-786).  float64 audio: the float64 interior, complex128.
 * Host faces split `lead` over the device list (smx_set_devices) like every batch call.                         */
int smx_hpss_masks_f32(const float *s, int64_t lead, int64_t bins, int64_t frames, int64_t kernel_h, int64_t kernel_p,
                       double power, double margin_h, double margin_p, float *mask_h, float *mask_p);
int smx_hpss_masks_f64(const double *s, int64_t lead, int64_t bins, int64_t frames, int64_t kernel_h, int64_t kernel_p,
                       double power, double margin_h, double margin_p, double *mask_h, double *mask_p);
int smx_hpss_masks_f32_dev(const float *d_s, int64_t lead, int64_t bins, int64_t frames, int64_t kernel_h,
                           int64_t kernel_p, double power, double margin_h, double margin_p, float *d_mask_h,
                           float *d_mask_p, void *stream);
int smx_hpss_of_spectrogram_f32(const float *s, int64_t lead, int64_t bins, int64_t frames, int64_t kernel_h,
                                int64_t kernel_p, double power, double margin_h, double margin_p, float *h, float *p);
int smx_hpss_of_spectrogram_f64(const double *s, int64_t lead, int64_t bins, int64_t frames, int64_t kernel_h,
                                int64_t kernel_p, double power, double margin_h, double margin_p, double *h, double *p);
int smx_hpss_of_spectrogram_f32_dev(const float *d_s, int64_t lead, int64_t bins, int64_t frames, int64_t kernel_h,
                                    int64_t kernel_p, double power, double margin_h, double margin_p, float *d_h,
                                    float *d_p, void *stream);
int smx_hpss_of_stft_c64(const float *z_c64, int64_t lead, int64_t bins, int64_t frames, int64_t kernel_h,
                         int64_t kernel_p, double power, double margin_h, double margin_p, float *z_h, float *z_p);
int smx_hpss_of_stft_c128(const double *z_c128, int64_t lead, int64_t bins, int64_t frames, int64_t kernel_h,
                          int64_t kernel_p, double power, double margin_h, double margin_p, double *z_h, double *z_p);
int smx_hpss_of_stft_c64_dev(const float *d_z_c64, int64_t lead, int64_t bins, int64_t frames, int64_t kernel_h,
                             int64_t kernel_p, double power, double margin_h, double margin_p, float *d_z_h,
                             float *d_z_p, void *stream);
int smx_hpss_f32(const smx_stft_config *c, const float *x, int64_t lead, int64_t n, int64_t kernel_h, int64_t kernel_p,
                 double power, double margin_h, double margin_p, float *y_h, float *y_p);
int smx_hpss_f64(const smx_stft_config *c, const double *x, int64_t lead, int64_t n, int64_t kernel_h, int64_t kernel_p,
                 double power, double margin_h, double margin_p, double *y_h, double *y_p);
int smx_hpss_f32_dev(const smx_stft_config *c, const float *d_x, int64_t lead, int64_t n, int64_t kernel_h,
                     int64_t kernel_p, double power, double margin_h, double margin_p, float *d_y_h, float *d_y_p,
                     void *stream);

/* ---- Effects: phase vocoder, time stretch, pitch shift (effects.ml, effects.mli:137-254) -------------------
 * The phase vocoder maps a complex spectrum z [lead; bins; frames] (the layout smx_stft_transform writes) to
 * [lead; bins; count], count = frames == 0 ? 0 : ceil(frames / rate) (effects.ml:90-92).  Output frame i sits at analysis
 * position i * rate: magnitudes interpolated between frames i0 = trunc(i * rate) and i0 + 1, phase an accumulator
 * advanced per output frame by omega_k + pv(arg z[k, i0 + 1] - arg z[k, i0] - omega_k) (effects.ml:189-229); the two rows
 * past the end read as silence.  SMX_PHASE_LOCKED adds identity phase locking (effects.ml:146-182).  The arithmetic is
 * float64 in the reference's operation order whatever the dtype of z and whatever smx_set_interior says, rounded once
 * into the dtype of z.  Only fft_size and hop of the stft config are read; bins must be fft_size / 2 + 1.  The locked
 * mode holds one frame's bins in LDS: up to 4083 bins (fft 8164), SMX_FAILURE beyond.
 *
 * smx_phase_vocoder_frames    effects.ml:90-92   the output frame count; no device
 * smx_time_stretch_length     effects.ml:295     rint(n / rate), ties to even; no device
 * smx_semitones               effects.ml:345-386 the best rational num/den for 2^(n / bins_per_octave) with neither term
 *                                                above 512: denominators 1..512, error compared in log2, the first best
 *                                                kept, reduced; no device
 * smx_phase_vocoder_*         effects.ml:285-289 `phase_vocoder`: checks of :96-117 (rate finite and positive, the bin axis)
 * smx_time_stretch_*          effects.ml:291-298 `time_stretch`: x [lead; n] -> y [lead; rint(n / rate)]: Stft.transform ->
 *                                                vocoder -> Stft.invert ~length, bit for bit those three calls, the
 *                                                spectra on the device in clip chunks.  float64 audio, and float32 audio
 *                                                under SMX_INTERIOR_F64 (widened first, rounded once at the end), keep
 *                                                complex128 spectra between the stages.  Also raises what Stft.invert
 *                                                raises (stft.ml:745-786).
 * smx_pitch_shift_*           effects.ml:324-334 `pitch_shift`: r is the resample config built for num -> den
 *                                                (smx_resample_config_create(num, den, ...)): time_stretch at the very
 *                                                quotient (double)den / (double)num, Resample.apply, cut or zero-extended
 *                                                to n.  DEVIATION: the conversion is float32 (smx_resample_apply_f32);
 *                                                float64 audio is stretched in float64, converted in float32, widened.  */
#define SMX_PHASE_INDEPENDENT 0
#define SMX_PHASE_LOCKED 1
int smx_phase_vocoder_frames(int64_t frames, double rate, int64_t *count);
int smx_time_stretch_length(int64_t n, double rate, int64_t *length);
int smx_semitones(double n, int64_t bins_per_octave, int64_t *num, int64_t *den);
int smx_phase_vocoder_c64(const smx_stft_config *c, const float *z_c64, int64_t lead, int64_t bins, int64_t frames,
                          double rate, int phase, float *out_c64);
int smx_phase_vocoder_c128(const smx_stft_config *c, const double *z_c128, int64_t lead, int64_t bins, int64_t frames,
                           double rate, int phase, double *out_c128);
int smx_phase_vocoder_c64_dev(const smx_stft_config *c, const float *d_z_c64, int64_t lead, int64_t bins, int64_t frames,
                              double rate, int phase, float *d_out_c64, void *stream);
int smx_phase_vocoder_c128_dev(const smx_stft_config *c, const double *d_z_c128, int64_t lead, int64_t bins,
                               int64_t frames, double rate, int phase, double *d_out_c128, void *stream);
int smx_time_stretch_f32(const smx_stft_config *c, const float *x, int64_t lead, int64_t n, double rate, int phase,
                         float *y);
int smx_time_stretch_f64(const smx_stft_config *c, const double *x, int64_t lead, int64_t n, double rate, int phase,
                         double *y);
int smx_time_stretch_f32_dev(const smx_stft_config *c, const float *d_x, int64_t lead, int64_t n, double rate, int phase,
                             float *d_y, void *stream);
int smx_pitch_shift_f32(const smx_stft_config *c, const smx_resample_config *r, int phase, const float *x, int64_t lead,
                        int64_t n, float *y);
int smx_pitch_shift_f64(const smx_stft_config *c, const smx_resample_config *r, int phase, const double *x, int64_t lead,
                        int64_t n, double *y);
int smx_pitch_shift_f32_dev(const smx_stft_config *c, const smx_resample_config *r, int phase, const float *d_x,
                            int64_t lead, int64_t n, float *d_y, void *stream);

/* ---- Chroma over a linear-frequency spectrum (chroma.ml:95-317; Soundml.chroma_stft, soundml.ml:97-107) --
 * Config: the float64 [n_chroma; bins] projection of chroma.ml:109-175 (Gaussian bumps in the wrapped
 * chroma distance, unit euclidean columns, optional octave envelope, rows rolled so row 0 is C).
 * apply: out = cast(normalise(W x cast_f64(s))) with the per-frame norm of chroma.ml:58-88: lengths below
 * the smallest normal of the dtype of s divide by 1.  s is [lead; bins; frames], out [lead; n_chroma; frames].
 * chroma_stft = apply . Stft.power_spectrum ~power (fft sizes must agree).                                 */
#define SMX_CHROMA_NORM_NONE 0
#define SMX_CHROMA_NORM_INF 1
#define SMX_CHROMA_NORM_P 2      /* norm_p: finite, positive */
int smx_chroma_config_create(int64_t n_chroma, double tuning, double ctroct, int has_octwidth, double octwidth,
                             int base_c, int64_t sample_rate, int64_t fft_size, smx_chroma_config **out);
void smx_chroma_config_destroy(smx_chroma_config *c);
int64_t smx_chroma_config_n_chroma(const smx_chroma_config *c);
int64_t smx_chroma_config_bins(const smx_chroma_config *c);
int64_t smx_chroma_config_fft_size(const smx_chroma_config *c);
int smx_chroma_filterbank(const smx_chroma_config *c, double *out /* [n_chroma; bins] */); /* chroma.ml:259 */
int smx_chroma_apply_f32(const smx_chroma_config *c, const float *s, int64_t lead, int64_t bins, int64_t frames,
                         int norm, double norm_p, float *out);
int smx_chroma_apply_f64(const smx_chroma_config *c, const double *s, int64_t lead, int64_t bins, int64_t frames,
                         int norm, double norm_p, double *out);
int smx_chroma_apply_f32_dev(const smx_chroma_config *c, const float *d_s, int64_t lead, int64_t bins,
                             int64_t frames, int norm, double norm_p, float *d_out, void *stream);
int smx_chroma_stft_f32(const smx_stft_config *sc, const smx_chroma_config *cc, const float *x, int64_t lead,
                        int64_t n, double power, int norm, double norm_p, float *out);
int smx_chroma_stft_f64(const smx_stft_config *sc, const smx_chroma_config *cc, const double *x, int64_t lead,
                        int64_t n, double power, int norm, double norm_p, double *out);
int smx_chroma_stft_f32_dev(const smx_stft_config *sc, const smx_chroma_config *cc, const float *d_x,
                            int64_t lead, int64_t n, int64_t x_stride, double power, int norm, double norm_p,
                            float *d_out, void *stream);

/* ---- Cqt: the offline constant-Q / variable-Q transform (cqt.ml:121-692, cqt.mli:64-315) --------------------------
 * Config (cqt.ml:287-424; no device needed): the octave-by-octave frequency ladder, relative bandwidths, fractional
 * filter lengths, main-lobe cutoff and its Nyquist check, the early decimations and the octave plan, all in float64 with
 * the reference's validation and Invalid_argument messages.  Octave i (highest first) holds `count` filters from global
 * bin `first`, analysed at `hop` on the signal halved `early + halvings` times by Resample.Config.create(2, 1, `High`)
 * through an n_fft-point rectangular centered frame.  Instead of the half-spectrum matrix K of `octave_kernel`
 * (cqt.ml:202-247) the config keeps its time-domain form with the octave gain folded in,
 *   g[b, n] = sum_{k <= n_fft / 2} K[b, k] exp(-2 pi i k n / n_fft),  so that  K . rfft(frame) = sum_n frame[n] g[b, n],
 * and the device projects every frame against g in float64 with no transform (cqt.hip).
 * gamma: SMX_CQT_GAMMA_FIXED reads gamma_value (finite, non-negative).  window / window_param as smx_window_make_param.
 * DEVIATION: float32 audio only (the reference also decimates float64).  The streaming face is smx_cqt_kernel_* below. */
typedef struct smx_cqt_config smx_cqt_config;
#define SMX_CQT_GAMMA_CONSTANT_Q 0
#define SMX_CQT_GAMMA_ERB 1
#define SMX_CQT_GAMMA_FIXED 2
int smx_cqt_config_create(int64_t n_bins, int64_t sample_rate, double fmin, int64_t bins_per_octave, int gamma, double gamma_value,
                          double tuning, double filter_scale, double norm, int window, double window_param, int scale, int64_t hop,
                          int pad, double pad_value, smx_cqt_config **out);                    /* cqt.ml:287-424 */
void smx_cqt_config_destroy(smx_cqt_config *c);
int64_t smx_cqt_config_n_bins(const smx_cqt_config *c);                                        /* cqt.mli:145-194 */
int64_t smx_cqt_config_bins_per_octave(const smx_cqt_config *c);
int64_t smx_cqt_config_sample_rate(const smx_cqt_config *c);
int64_t smx_cqt_config_hop(const smx_cqt_config *c);
int64_t smx_cqt_config_n_octaves(const smx_cqt_config *c);
int64_t smx_cqt_config_early(const smx_cqt_config *c);    /* 2:1 decimations before octave zero (cqt.ml:338-345) */
int64_t smx_cqt_config_latency(const smx_cqt_config *c);  /* cqt.mli:196-231, K = smx_resample_config_latency of the 2:1 plan */
double smx_cqt_config_cutoff(const smx_cqt_config *c);
int smx_cqt_frequencies(const smx_cqt_config *c, double *out /* [n_bins] */);                  /* cqt.mli:243 */
int smx_cqt_filter_lengths(const smx_cqt_config *c, double *out /* [n_bins] */);               /* cqt.mli:257 */
int smx_cqt_frames(const smx_cqt_config *c, int64_t n, int64_t *frames);                       /* cqt.mli:278 */
/* the plan, for inspection: octave i's extents; its taps g as [count; n_fft] interleaved (re, im) float64; the [n_bins]
 * `scale` divisors, sqrt of the filter lengths at the rate octave zero runs at (all ones when scale is off) */
int smx_cqt_config_octave(const smx_cqt_config *c, int64_t i, int64_t *first, int64_t *count, int64_t *n_fft, int64_t *hop,
                          int64_t *halvings);
int smx_cqt_config_taps(const smx_cqt_config *c, int64_t i, double *out);
int smx_cqt_config_divisors(const smx_cqt_config *c, double *out);
/* transform (cqt.mli:285-303): x [lead; n] float32 -> [lead; n_bins; frames] complex64 (interleaved), float64 inside,
 * one rounding.  power_spectrum (cqt.mli:305-315): |transform|^power in float32, the magnitude taken of the rounded
 * complex64 value as the reference does.  Zero lead or zero frames: nothing is written. */
int smx_cqt_transform_f32(const smx_cqt_config *c, const float *x, int64_t lead, int64_t n, float *out_c64);
int smx_cqt_transform_f32_dev(const smx_cqt_config *c, const float *d_x, int64_t lead, int64_t n, int64_t x_stride, float *d_out_c64,
                              void *stream);
int smx_cqt_power_spectrum_f32(const smx_cqt_config *c, const float *x, int64_t lead, int64_t n, double power, float *out);
int smx_cqt_power_spectrum_f32_dev(const smx_cqt_config *c, const float *d_x, int64_t lead, int64_t n, int64_t x_stride, double power,
                                   float *d_out, void *stream);
/* diagnostics (tests of the projection kernel alone, on exact data): one launch of the strided filter-bank projection
 *   z[c, first + b, p] = sum_{n < n_fft} src(c, p hop - n_fft / 2 + n) g[b, n] / divisor[b],   b < count, p < frames,
 * with caller-supplied device taps d_taps [count; n_fft] (re, im) float64 and optional d_divisors [count]; src is
 * d_x [lead; n] float32 under the boundary rule `pad` of Stft's centered alignment; the result lands in rows
 * [first, first + count) of d_out [lead; n_bins; frames]: complex64 (as_power == 0) or |z|^power float32 */
int smx_debug_cqt_project_f32_dev(const float *d_x, int64_t lead, int64_t n, int64_t x_stride, const double *d_taps,
                                  const double *d_divisors, int64_t count, int64_t n_fft, int64_t hop, int pad, double pad_value,
                                  int64_t first, int64_t n_bins, int64_t frames, int as_power, double power, void *d_out,
                                  void *stream);
/* ---- Cqt.Kernel: the streaming transform (cqt.mli:317-413, cqt.ml:694-1012) ------------------------------------------
 * One state for all channels: a streaming 2:1 decimator (smx_resample_stream_*) per early decimation and per halving
 * octave, per octave a device ring of its float32 stream, and one ring of finished columns.  The law is stronger than the
 * reference's (which anchors on the kernel's own one-chunk run and documents 2e-6 against the offline transform): the
 * concatenation of every step's columns plus the flush's equals smx_cqt_transform_f32 (with a power:
 * smx_cqt_power_spectrum_f32) of the concatenated signal BIT FOR BIT under every chunking, because the projection is one
 * fixed fma chain per (frame, bin) whichever kernel runs it and the decimator is bit-equal to its offline face.
 * The schedule is host arithmetic and needs no device:
 *   columns_ready  the columns that have left once `fed` samples went in (cqt.mli:199-231): frame p of octave i is projected
 *                  when its stream holds p hop_i + n_fft_i / 2 samples (one more for frame 0 under Reflect, which reads the
 *                  mirror of its first sample); a column leaves when every octave has projected it.  For Constant and Edge
 *                  padding this is max(0, (fed - latency) / hop + 1).
 *   column_bound   the most columns one step of at most max_block samples, or the flush, returns.
 *   run_ahead      the most columns an octave can be ahead of the slowest one (cqt.mli:381-383); the column ring holds
 *                  run_ahead + column_bound. */
typedef struct smx_cqt_kernel smx_cqt_kernel;
int smx_cqt_config_columns_ready(const smx_cqt_config *c, int64_t fed, int64_t *columns);
int smx_cqt_config_column_bound(const smx_cqt_config *c, int64_t max_block, int64_t *bound);
int smx_cqt_config_run_ahead(const smx_cqt_config *c, int64_t *columns);
/* prepare (cqt.mli:370-388): Invalid_argument for channels < 1 or max_block < 1, checked before any device is touched.
 * has_power != 0: the kernel emits |z|^power in float32 instead of complex64.  The config must outlive the kernel. */
int smx_cqt_kernel_prepare(const smx_cqt_config *c, int64_t channels, int64_t max_block, int has_power, double power,
                           smx_cqt_kernel **out);
void smx_cqt_kernel_destroy(smx_cqt_kernel *k);
int smx_cqt_kernel_reset(smx_cqt_kernel *k);                                                    /* cqt.mli:411-412 */
/* host arithmetic: the columns a step of n samples would return now, and what the flush would (size the output by them) */
int64_t smx_cqt_kernel_columns_after(const smx_cqt_kernel *k, int64_t n);
int64_t smx_cqt_kernel_pending(const smx_cqt_kernel *k);
/* step (cqt.mli:390-400): x [channels; n] float32 with x_stride; the completed columns land in out [channels; n_bins;
 * out_stride] (complex64 interleaved, or float32 under a power) and *columns says how many.  Invalid_argument: a drained
 * kernel, n > max_block.  n = 0 does nothing.  The _dev form enqueues on `stream` and never synchronises.
 * flush (cqt.mli:402-409): drains the decimators front to back, projects the remaining frames under the right boundary
 * rule and returns every column up to smx_cqt_frames of the total; a second flush returns none. */
int smx_cqt_kernel_step_f32(smx_cqt_kernel *k, const float *x, int64_t n, int64_t x_stride, void *out, int64_t out_stride,
                            int64_t *columns);
int smx_cqt_kernel_flush_f32(smx_cqt_kernel *k, void *out, int64_t out_stride, int64_t *columns);
int smx_cqt_kernel_step_f32_dev(smx_cqt_kernel *k, const float *d_x, int64_t n, int64_t x_stride, void *d_out, int64_t out_stride,
                                int64_t *columns, void *stream);
int smx_cqt_kernel_flush_f32_dev(smx_cqt_kernel *k, void *d_out, int64_t out_stride, int64_t *columns, void *stream);
/* Chroma over a constant-Q spectrum (chroma.ml:324-385; Soundml.chroma_cqt).  cqt_projection: the 0/1 fold
 * [n_chroma; n_bins] (bins_per_octave must be a multiple of n_chroma).  of_cqt: fold + the per-frame normalisation of
 * smx_chroma_apply.  chroma_cqt = of_cqt . Cqt.power_spectrum ~power:1; the magnitudes stay on the device. */
int smx_chroma_cqt_projection(const smx_cqt_config *c, int64_t n_chroma, double *out /* [n_chroma; n_bins] */);
int smx_chroma_of_cqt_f32(const smx_cqt_config *c, const float *s, int64_t lead, int64_t bins, int64_t frames, int64_t n_chroma,
                          int norm, double norm_p, float *out);
int smx_chroma_of_cqt_f64(const smx_cqt_config *c, const double *s, int64_t lead, int64_t bins, int64_t frames, int64_t n_chroma,
                          int norm, double norm_p, double *out);
int smx_chroma_of_cqt_f32_dev(const smx_cqt_config *c, const float *d_s, int64_t lead, int64_t bins, int64_t frames, int64_t n_chroma,
                              int norm, double norm_p, float *d_out, void *stream);
int smx_chroma_cqt_f32(const smx_cqt_config *c, const float *x, int64_t lead, int64_t n, int64_t n_chroma, int norm, double norm_p,
                       float *out);
int smx_chroma_cqt_f32_dev(const smx_cqt_config *c, const float *d_x, int64_t lead, int64_t n, int64_t x_stride, int64_t n_chroma,
                           int norm, double norm_p, float *d_out, void *stream);

/* ---- Least-squares synthesis: Stft.invert (stft.ml:902-939, stft.mli "invert") --------------------
 * x[m] = (sum_p w[m - p hop] irfft(Z[:, p])[m - p hop]) / (sum_p w^2[m - p hop]) in padded coordinates,
 * boundary extension trimmed, cut or zero-extended to `length`.  z is [lead; bins; frames] complex
 * (interleaved re, im; frames fastest), out is [lead; out_len] with out_len = length when has_length,
 * else smx_stft_output_length(frames).  The imaginary parts of the DC and Nyquist bins are ignored.
 * Invalid_argument (messages of stft.ml:745-786): wrong bin count, negative length, a window / hop pair
 * whose overlap-added squared window does not stay above 1e-10 of its maximum (smx_stft_nola).        */
int smx_stft_nola(const smx_stft_config *c, int *invertible);                         /* stft.ml:731-743 */
int smx_stft_output_length(const smx_stft_config *c, int64_t frames, int64_t *length); /* stft.ml:792-796 */
int smx_stft_invert_f32(const smx_stft_config *c, const float *z_c64, int64_t lead, int64_t bins,
                        int64_t frames, int has_length, int64_t length, float *out);
int smx_stft_invert_f64(const smx_stft_config *c, const double *z_c128, int64_t lead, int64_t bins,
                        int64_t frames, int has_length, int64_t length, double *out);
int smx_stft_invert_f32_dev(const smx_stft_config *c, const float *d_z_c64, int64_t lead, int64_t bins,
                            int64_t frames, int has_length, int64_t length, float *d_out, void *stream);
int smx_stft_invert_f64_dev(const smx_stft_config *c, const double *d_z_c128, int64_t lead, int64_t bins,
                            int64_t frames, int has_length, int64_t length, double *d_out, void *stream);

/* ---- FIR block convolution (BASELINE config 4; model resample.ml:383-415) --
 * y[c][i] = sum_k h[k] x[c][i-k], zeros before the stream start, i in [0, n).
 * Overlap-save on the library's own FFT core, spectrum of h precomputed.     */
int smx_fir_kaiser_beta(double attenuation_db, double *out);            /* resample.ml:105-109 */
int smx_fir_design_lowpass(int64_t taps, double cutoff, double beta, double *h); /* :145-163 */
int smx_fir_plan_create(const double *h, int64_t taps, smx_fir_plan **out);
void smx_fir_plan_destroy(smx_fir_plan *p);
int64_t smx_fir_plan_block(const smx_fir_plan *p);                      /* FFT length N */
int smx_fir_apply_f32(const smx_fir_plan *p, const float *x, int64_t channels, int64_t n, float *y);
int smx_fir_apply_f32_dev(const smx_fir_plan *p, const float *d_x, int64_t channels, int64_t n,
                          int64_t x_stride, float *d_y, int64_t y_stride, void *stream);


/* ---- Resample: the overlap-save executor's pieces ------------------------------------------------
 * The reference's planner, polyphase bank and cascade logic (resample.ml, 2100 lines) stay in OCaml; what moves to the
 * device is the block convolution of a stage and the block identity its own C stub computes.
 *
 * smx_resample_ols_geom    resample.ml:279-300 `ols_block_n` / `ols_geom`: (N, B, delta) of a xL or /M stage of group
 *                          delay K consuming `rate` Hz; *eligible = 0 past the 130 ms emission ceiling.
 * smx_resample_prototype   resample.ml:145-163 `design_prototype`: the 2 K L + 1 tap Kaiser-sinc, float64, sum = L.
 * smx_resample_shape_c128  replaces `soundml_resample_shape` (resample_stubs.c:329-422; bound in resample.ml:1186-1196
 *                          as `resample_shape_c`): interleaved complex128 half spectra x [lines; N/2+1] and plan
 *                          spectrum h -> y [lines; W/2+1], W = N sl | N / sm | N.  xL: periodic extension times h[k];
 *                          /M: product on the half grid, alias fold in ascending order.  Same operations in the same
 *                          order in float64 (no fused multiply-add): bit for bit the stub's result.  Geometry errors
 *                          are Failure with the stub's message ("soundml_resample_shape: invalid geometry").
 * smx_resample_stage_*     one stage y[i] = sum_t proto[t] xu[i M + K L - t], xu = x zero-stuffed by L, ceil(n L / M)
 *                          outputs (what `ols_run` + the virtual-silence drain emit, resample.ml:1456-1599,1745-1755),
 *                          float32 interior.  A pure xL or /M stage (the overlap-save eligible ones, resample.ml:279-300)
 *                          runs in its polyphase form block by block in the frequency domain -- L filters of the input at
 *                          the input rate / the sum of M filters of the input's phases at the output rate: the arithmetic
 *                          of the reference's spectral shortcut (resample_stubs.c:329-372) regrouped into power-of-two
 *                          transforms at the low rate; any other L / M as one block convolution at the interpolated
 *                          rate on the FIR kernel.  2 K L + 1 <= 16384 taps.
 * smx_resample_kernel_*    `Resample.Kernel.{prepare,step,flush,reset}` (resample.mli:270-319, executor `ols_run`
 *                          resample.ml:1456-1599) of ONE pure xL or /M stage: all channels in one state, the unconsumed
 *                          input (the block carry) on the device; a step emits the block pairs its samples complete
 *                          (burst emission, possibly nothing), flush the virtual-silence tail, and every partition of a
 *                          signal totals smx_resample_stage_apply bit for bit.  Errors as the reference's: a chunk
 *                          longer than max_block, a step after flush (reset first), channels or max_block < 1 are
 *                          SMX_INVALID_ARGUMENT.  The stage must outlive the kernel.  A second flush emits nothing.     */
int smx_resample_ols_geom(int64_t rate, int64_t l, int64_t m, int64_t k, int64_t *n, int64_t *b, int64_t *delta,
                          int *eligible);
int smx_resample_prototype(int64_t l, int64_t k, double fc, double beta, double *h /* 2 K L + 1 */);
int smx_resample_shape_c128(const double *x, const double *h, double *y, int64_t lines, int64_t n, int64_t sl, int64_t sm);
int smx_resample_shape_c128_dev(const double *d_x, const double *d_h, double *d_y, int64_t lines, int64_t n, int64_t sl,
                                int64_t sm, void *stream);
int smx_resample_stage_create(const double *proto /* 2 K L + 1 */, int64_t l, int64_t m, int64_t k, smx_resample_stage **out);
void smx_resample_stage_destroy(smx_resample_stage *s);
int64_t smx_resample_stage_out_length(const smx_resample_stage *s, int64_t n);       /* ceil(n L / M) */
int smx_resample_stage_streams(const smx_resample_stage *s);   /* 1: runs as polyphase blocks, so smx_resample_kernel_prepare takes it */
int smx_resample_stage_apply_f32(const smx_resample_stage *s, const float *x, int64_t channels, int64_t n, float *y);
int smx_resample_stage_apply_f32_dev(const smx_resample_stage *s, const float *d_x, int64_t channels, int64_t n,
                                     int64_t x_stride, float *d_y, int64_t y_stride, void *stream);
int smx_resample_kernel_prepare(const smx_resample_stage *s, int64_t channels, int64_t max_block, smx_resample_kernel **out);
void smx_resample_kernel_destroy(smx_resample_kernel *k);
int smx_resample_kernel_reset(smx_resample_kernel *k);
int64_t smx_resample_kernel_out_bound(const smx_resample_kernel *k, int64_t n);   /* most samples per channel a step of n can emit */
int64_t smx_resample_kernel_pending(const smx_resample_kernel *k);                /* samples per channel the next flush emits */
/* x [channels; n] (row stride x_stride) -> y [channels; *n_out] (row stride y_stride >= out_bound(n) / pending) */
int smx_resample_kernel_step_f32(smx_resample_kernel *k, const float *x, int64_t n, int64_t x_stride, float *y, int64_t y_stride,
                                 int64_t *n_out);
int smx_resample_kernel_flush_f32(smx_resample_kernel *k, float *y, int64_t y_stride, int64_t *n_out);
int smx_resample_kernel_step_f32_dev(smx_resample_kernel *k, const float *d_x, int64_t n, int64_t x_stride, float *d_y,
                                     int64_t y_stride, int64_t *n_out, void *stream);
int smx_resample_kernel_flush_f32_dev(smx_resample_kernel *k, float *d_y, int64_t y_stride, int64_t *n_out, void *stream);

/* ---- Resample.Config / Resample.apply: arbitrary-ratio conversion (resample.mli:91-197) -----------------------------
 * smx_resample_config_create    resample.ml:872-939 `Config.create`: validation in the reference's order and wording
 *                               (sample_rate, target, attenuation in [40, 200], passband in [0.5, 0.99]); g = gcd,
 *                               L = target / g, M = sample_rate / g; L = M = 1 is the identity (latency 0, no filter);
 *                               otherwise the single-stage design of :919-932 (width (1 - passband) / max(L, M),
 *                               kaiser_numtaps :113-116, K = max(1, ceil((taps - 1) / 2 L)), fc mid-transition, Kaiser
 *                               beta) on smx_resample_prototype.  A bank of L (2 K + 1) 8 bytes over the 8 MiB budget
 *                               (:230, :924-925) is SMX_INVALID_ARGUMENT with the message of :997-1011, clock-drift
 *                               hint included.  attenuation / passband are read for SMX_RESAMPLE_CUSTOM only.  No
 *                               device is needed.  DEVIATION: every conversion is ONE stage; the two-stage cascade
 *                               search (`plan_cascade`, :540-870) is not restated, so the ratios the reference
 *                               cascades run its `cost_single` design here: same spec, another latency.
 * smx_resample_config_executor  SMX_RESAMPLE_OLS exactly for a pure x2..4 or /2..4 stage (:951) that
 *                               smx_resample_ols_geom reports eligible: the polyphase-block stage above on this
 *                               prototype (smx_resample_config_stage; owned by the config).  SMX_RESAMPLE_DIRECT for
 *                               every other ratio: the polyphase dot product of :1318-1326, 2 K + 1 multiply-adds per
 *                               output, float32 bank (rounded once, uploaded per device on first use).
 * smx_resample_config_*         sample_rate, target, quality (:1021-1025); l / m = `rate` (:1027); latency = K in input
 *                               samples (:1029); output_latency = K L / M reduced (:1031-1036); output_frames =
 *                               ceil(n L / M), n < 0 is SMX_INVALID_ARGUMENT (:1038-1051); prototype: a float64 copy,
 *                               prototype_length = 2 K L + 1 long (:1053-1056); design: the stage's (fc, beta).
 * smx_resample_apply_f32[_dev]  `Resample.apply` (resample.mli:176-197, resample.ml:1318-1326) on float32: x [channels; n]
 *                               -> y [channels; ceil(n L / M)], y[i] = sum_j bank[p_i][j] x[q_i - j], zeros outside the
 *                               stream.  Every output is summed in one fixed order, so a batch equals its rows, a strided
 *                               input its copy and any streaming partition the whole, bit for bit.
 * smx_resample_stream_*         `Resample.Kernel.{prepare,step,flush,reset}` (resample.mli:270-319) of a DIRECT config: the
 *                               last 2 K samples of every channel stay on the device; after `fed` samples in total the
 *                               steps have emitted max(0, ceil((fed - K) L / M)) (`ready`, resample.ml:1298), flush the
 *                               rest up to ceil(fed L / M).  Errors as smx_resample_kernel_*.  The config must outlive
 *                               the kernel.  (An OLS config streams through smx_resample_kernel_* on its stage.)          */
int smx_resample_config_create(int64_t sample_rate, int64_t target, int quality, double attenuation, double passband,
                               smx_resample_config **out);
void smx_resample_config_destroy(smx_resample_config *c);
int64_t smx_resample_config_sample_rate(const smx_resample_config *c);
int64_t smx_resample_config_target(const smx_resample_config *c);
int smx_resample_config_quality(const smx_resample_config *c, double *attenuation, double *passband);   /* returns SMX_RESAMPLE_* */
int64_t smx_resample_config_l(const smx_resample_config *c);
int64_t smx_resample_config_m(const smx_resample_config *c);
int64_t smx_resample_config_latency(const smx_resample_config *c);
int smx_resample_config_executor(const smx_resample_config *c);
const smx_resample_stage *smx_resample_config_stage(const smx_resample_config *c);   /* NULL unless SMX_RESAMPLE_OLS */
int smx_resample_config_design(const smx_resample_config *c, double *fc, double *beta);
int smx_resample_config_output_latency(const smx_resample_config *c, int64_t *num, int64_t *den);
int smx_resample_config_output_frames(const smx_resample_config *c, int64_t n, int64_t *out);
int64_t smx_resample_config_prototype_length(const smx_resample_config *c);
int smx_resample_config_prototype(const smx_resample_config *c, double *h /* prototype_length */);
int smx_resample_apply_f32(const smx_resample_config *c, const float *x, int64_t channels, int64_t n, float *y);
int smx_resample_apply_f32_dev(const smx_resample_config *c, const float *d_x, int64_t channels, int64_t n, int64_t x_stride,
                               float *d_y, int64_t y_stride, void *stream);
int smx_resample_stream_prepare(const smx_resample_config *c, int64_t channels, int64_t max_block, smx_resample_stream **out);
void smx_resample_stream_destroy(smx_resample_stream *k);
int smx_resample_stream_reset(smx_resample_stream *k);
int64_t smx_resample_stream_out_bound(const smx_resample_stream *k, int64_t n);   /* most samples per channel a step of n can emit */
int64_t smx_resample_stream_pending(const smx_resample_stream *k);                /* samples per channel the next flush emits */
int smx_resample_stream_step_f32(smx_resample_stream *k, const float *x, int64_t n, int64_t x_stride, float *y, int64_t y_stride,
                                 int64_t *n_out);
int smx_resample_stream_flush_f32(smx_resample_stream *k, float *y, int64_t y_stride, int64_t *n_out);
int smx_resample_stream_step_f32_dev(smx_resample_stream *k, const float *d_x, int64_t n, int64_t x_stride, float *d_y,
                                     int64_t y_stride, int64_t *n_out, void *stream);
int smx_resample_stream_flush_f32_dev(smx_resample_stream *k, float *d_y, int64_t y_stride, int64_t *n_out, void *stream);

/* ---- Iir: recursive filters as cascaded second-order sections (scipy.signal.sosfilt / sosfilt_zi / sosfiltfilt; the
 * reference lists "IIR/FIR filtering" as planned and has no such module) -----------------------------------------------------
 * sos is [S; 6] float64 with rows b0 b1 b2 a0 a1 a2, 1 <= S <= smx_iir_max_sections() = 8, every a0 exactly 1.0, all finite.
 * Audio x [lead; n] -> y [lead; n].  One step of the cascade on a sample u, in float64, every product and every sum rounded
 * on its own (no fused operation), for k = 0 .. S-1 in turn:
 *     y = b0 u + z[k][0];   z[k][0] = (b1 u - a1 y) + z[k][1];   z[k][1] = b2 u - a2 y;   u = y
 * Run serially from a zero state this is sosfilt's float64 output bit for bit.  A state is [S; 2] float64, z[k][0], z[k][1].
 *
 * The stated order, shared bit for bit by both kernels, the host faces and the stream kernel.  Time is cut
 * into blocks of B = smx_iir_block() = 256 samples counted from the first sample of the call (of the stream since reset).
 * s_b is the state entering block b, s_0 = zi or zero.  The outputs of block b are the serial cascade run from s_b over the
 * block's samples; w_b is the end state of the same cascade over the same samples from a ZERO state;
 *     s_{b+1}[i] = (((M[i][0] s_b[0] + M[i][1] s_b[1]) + M[i][2] s_b[2]) + ...) + w_b[i]       ascending j, w_b last
 * with M [2S; 2S] built on the host (smx_iir_matrix, row-major): column i is the end state of B zero-input steps of the
 * cascade from the unit state e_i.  Outputs are rounded once, to the dtype of the input.  The state handed back (zf) is the
 * running state after the last sample: s_{b+1} where the call ends on a block edge.  A leading slice of a batch, both kernels
 * (SMX_DISABLE_FAST=1 forces the general one) and every chunking of the stream kernel give the same bits; a call continued
 * from another call's zf restarts the block grid and agrees to rounding only.
 *
 *   smx_iir_zi        the unit-step steady state in closed form, [S; 2]: per section g = (b0 + b1 + b2) / (1 + a1 + a2),
 *                     z[k][0] = g - b0, z[k][1] = b2 - a2 g, both times the product of the earlier sections' g
 *                     (sosfilt_zi to rounding).  A section with 1 + a1 + a2 == 0 is refused.
 *   smx_iir_apply_*   zi: NULL (zero state), [S; 2] (zi_rows 0) or [lead; S; 2] (zi_rows 1); zf: NULL or [lead; S; 2].
 *                     n = 0 hands zi back as zf.
 *   smx_iir_filtfilt_*  sosfiltfilt with its defaults: odd extension by padlen = 3 (2 S + 1 - min(#rows with b2 == 0,
 *                     #rows with a2 == 0)) samples on each side, 2 x[0] - x[padlen - i] and 2 x[n-1] - x[n-2-k] taken in
 *                     float64; a forward pass from zi times the extended signal's first sample; the float64 result reversed;
 *                     a second pass from zi times ITS first sample; reversed again, trimmed, rounded once.  Each pass's block
 *                     grid starts at that pass's first sample.  n <= padlen is refused.
 *   smx_iir_kernel_*  Iir.Kernel.{prepare, step, flush, reset}: 6 S doubles per channel stay on the device (s_b, the partial
 *                     w, the running state); the position inside the block is a host integer.  A step takes [channels; m]
 *                     and returns [channels; m] (latency zero) and may begin and end anywhere inside a block; the
 *                     concatenated steps equal smx_iir_apply_* of the whole signal bit for bit.  flush emits nothing and
 *                     drains the kernel: a step after it is refused until reset.  The kernel shares the configuration's
 *                     tables and may outlive the handle.
 *
 * The device-resident forms end in `_card_f32` (the placement and stream suites keep closed tables of the other endings; these
 * have tables and laws of their own: tests/test_gpu_placement_iir.py, tests/test_gpu_streams_iir.py) and take the stream
 * directly after the handle.  Rows of d_x lie x_stride >= n apart, results are dense.  smx_iir_apply_card_f32 takes the per-call
 * state zi from HOST memory (it travels with the launch) and the per-channel one, d_zi_rows, from device memory; at most one
 * of the two.  Everything is enqueued on `stream`; nothing synchronises it. */
typedef struct smx_iir smx_iir;
typedef struct smx_iir_kernel smx_iir_kernel;
int smx_iir_create(const double *sos, int64_t sections, smx_iir **out);
void smx_iir_destroy(smx_iir *c);
int64_t smx_iir_block(void);
int64_t smx_iir_span_blocks(void);       /* blocks a wave of the block route owns: 64 */
int64_t smx_iir_max_sections(void);
int64_t smx_iir_sections(const smx_iir *c);
int64_t smx_iir_padlen(const smx_iir *c);
int smx_iir_matrix(const smx_iir *c, double *m /* [2 S; 2 S] */);
int smx_iir_zi(const smx_iir *c, double *zi /* [S; 2] */);
int smx_iir_apply_f32(const smx_iir *c, const float *x, int64_t lead, int64_t n, const double *zi, int zi_rows, float *out,
                      double *zf);
int smx_iir_apply_f64(const smx_iir *c, const double *x, int64_t lead, int64_t n, const double *zi, int zi_rows, double *out,
                      double *zf);
int smx_iir_apply_card_f32(const smx_iir *c, void *stream, const float *d_x, int64_t lead, int64_t n, int64_t x_stride,
                           const double *zi, const double *d_zi_rows, float *d_out, double *d_zf);
int smx_iir_filtfilt_f32(const smx_iir *c, const float *x, int64_t lead, int64_t n, float *out);
int smx_iir_filtfilt_f64(const smx_iir *c, const double *x, int64_t lead, int64_t n, double *out);
int smx_iir_filtfilt_card_f32(const smx_iir *c, void *stream, const float *d_x, int64_t lead, int64_t n, int64_t x_stride,
                              float *d_out);
int smx_iir_kernel_prepare(const smx_iir *c, int64_t channels, smx_iir_kernel **out);
void smx_iir_kernel_destroy(smx_iir_kernel *k);
int smx_iir_kernel_reset(smx_iir_kernel *k);
int smx_iir_kernel_flush(smx_iir_kernel *k);
int64_t smx_iir_kernel_position(const smx_iir_kernel *k);   /* samples per channel since reset */
int smx_iir_kernel_step_f32(smx_iir_kernel *k, const float *x, int64_t m, float *out);
int smx_iir_kernel_step_f64(smx_iir_kernel *k, const double *x, int64_t m, double *out);
int smx_iir_kernel_step_card_f32(smx_iir_kernel *k, void *stream, const float *d_x, int64_t m, int64_t x_stride, float *d_out);

/* ---- Loudness: programme loudness and true peak (ITU-R BS.1770-4; the meter's windows and compliance signals: EBU Tech 3341;
 * the reference has no such module) ------------------------------------------------------------------------------------------
 * Audio is [clips; channels; n], time fastest, 1 <= channels <= smx_loudness_max_channels() = 32.  DESIGN.md 4.8l states every
 * order once; every face, both kernels and every chunking of the meter share it bit for bit.
 *
 *   smx_loudness_k_weighting   BS.1770-4 Annex 1: the shelf and the RLB high-pass as two second-order sections [2; 6] (rows
 *                     b0 b1 b2 1 a1 a2) designed from their analogue prototypes by the bilinear transform; at 48000 Hz the
 *                     recommendation's printed table.  rate < smx_loudness_min_rate() = 8000 is refused.
 *   the grid          BS.1770-4 Annex 1 gating blocks: step = smx_loudness_step(rate) = (rate + 5) / 10 samples (100 ms), a
 *                     block is 4 steps (400 ms, 75 % overlap), nb = smx_loudness_blocks(rate, n) whole blocks, a trailing partial
 *                     block is dropped.  Short-term windows (EBU Tech 3341: 3 s) are 30 steps at the same hop.
 *   smx_loudness_block_energy_*  z [clips; channels; nb] float64: the mean square of each channel's K-weighted signal over each
 *                     block (BS.1770-4 eq. 1).  The cascade runs in float64 from a zero state by Iir's stated order (4.8k); the
 *                     weighted signal is never rounded and never stored.
 *   smx_loudness_momentary_*   -0.691 + 10 log10(sum_c G_c z[c, j]) per block (BS.1770-4 eq. 2; EBU Tech 3341 momentary), or with
 *                     short_term != 0 over the 30-step windows: [clips; nb] or [clips; max(0, nb - 26)].  weights: host
 *                     [channels] or NULL (1.0 each).  A zero-energy block gives -inf.
 *   smx_loudness_integrated_*  BS.1770-4 eqs. 3-7: the absolute gate e > smx_loudness_absolute_gate() = 10^((-70 + 0.691) / 10),
 *                     the relative gate e > 0.1 mean(e through the absolute gate), -0.691 + 10 log10(mean of the blocks through
 *                     both); no such block: -inf.  mask: NULL, or [clips; nb] bytes: bit 0 through the absolute gate, bit 1 both.
 *   smx_loudness_true_peak_*   BS.1770-4 Annex 2 with the taps of smx_loudness_true_peak_taps (49-tap Kaiser sinc, 4x):
 *                     max_i,p |sum_j h[p + 4 j] x[i - j]| per row, zeros outside the signal, a linear amplitude.
 *   smx_loudness_normalize_*   one gain per clip, 10^((target - integrated) / 20), lowered until gain * max_c true_peak <=
 *                     ceiling when has_ceiling; a clip at -inf keeps gain 1.  Float64 on the device, one rounding.
 *   smx_loudness_meter_*  Loudness.Meter (EBU Tech 3341's live meter): per channel Iir's record, the open piece's partial sum and
 *                     the step energies so far stay on the device; the position is a host integer.  A step takes
 *                     [clips; channels; len] and returns the momentary loudness [clips; k] of the k blocks that completed,
 *                     k = max(0, (position + len) / step - 3) - max(0, position / step - 3).  read: what 0 = integrated
 *                     [clips], 1 = short-term [clips; max(0, blocks - 26)] of everything fed so far.
 *
 * The device-resident forms end in `_card_f32` and take the stream directly after the first argument (tables and laws of their
 * own: tests/test_gpu_placement_loudness.py, tests/test_gpu_streams_loudness.py).  Rows of d_x (one per clip and channel) lie
 * x_stride >= n apart, results are dense.  Everything is enqueued on `stream`; nothing synchronises it. */
typedef struct smx_loudness_meter smx_loudness_meter;
int64_t smx_loudness_min_rate(void);
int64_t smx_loudness_max_channels(void);
int64_t smx_loudness_step(int64_t rate);
int64_t smx_loudness_blocks(int64_t rate, int64_t n);
double smx_loudness_absolute_gate(void);
int smx_loudness_k_weighting(int64_t rate, double *sos /* [2; 6] */);
int smx_loudness_true_peak_taps(double *h /* [49] */);
int smx_loudness_block_energy_f32(const float *x, int64_t clips, int64_t channels, int64_t n, int64_t rate, double *z);
int smx_loudness_block_energy_f64(const double *x, int64_t clips, int64_t channels, int64_t n, int64_t rate, double *z);
int smx_loudness_block_energy_card_f32(const float *d_x, void *stream, int64_t clips, int64_t channels, int64_t n, int64_t x_stride,
                                       int64_t rate, double *d_z);
int smx_loudness_momentary_f32(const float *x, int64_t clips, int64_t channels, int64_t n, int64_t rate, const double *weights,
                               int short_term, float *out);
int smx_loudness_momentary_f64(const double *x, int64_t clips, int64_t channels, int64_t n, int64_t rate, const double *weights,
                               int short_term, double *out);
int smx_loudness_momentary_card_f32(const float *d_x, void *stream, int64_t clips, int64_t channels, int64_t n, int64_t x_stride,
                                    int64_t rate, const double *weights, int short_term, float *d_out);
int smx_loudness_integrated_f32(const float *x, int64_t clips, int64_t channels, int64_t n, int64_t rate, const double *weights,
                                float *out, unsigned char *mask);
int smx_loudness_integrated_f64(const double *x, int64_t clips, int64_t channels, int64_t n, int64_t rate, const double *weights,
                                double *out, unsigned char *mask);
int smx_loudness_integrated_card_f32(const float *d_x, void *stream, int64_t clips, int64_t channels, int64_t n, int64_t x_stride,
                                     int64_t rate, const double *weights, float *d_out, unsigned char *d_mask);
int smx_loudness_true_peak_f32(const float *x, int64_t rows, int64_t n, float *out);
int smx_loudness_true_peak_f64(const double *x, int64_t rows, int64_t n, double *out);
int smx_loudness_true_peak_card_f32(const float *d_x, void *stream, int64_t rows, int64_t n, int64_t x_stride, float *d_out);
int smx_loudness_normalize_f32(const float *x, int64_t clips, int64_t channels, int64_t n, int64_t rate, double target,
                               int has_ceiling, double ceiling, const double *weights, float *out);
int smx_loudness_normalize_f64(const double *x, int64_t clips, int64_t channels, int64_t n, int64_t rate, double target,
                               int has_ceiling, double ceiling, const double *weights, double *out);
int smx_loudness_normalize_card_f32(const float *d_x, void *stream, int64_t clips, int64_t channels, int64_t n, int64_t x_stride,
                                    int64_t rate, double target, int has_ceiling, double ceiling, const double *weights, float *d_out);
int smx_loudness_meter_prepare(int64_t rate, int64_t clips, int64_t channels, const double *weights, smx_loudness_meter **out);
void smx_loudness_meter_destroy(smx_loudness_meter *m);
int smx_loudness_meter_reset(smx_loudness_meter *m);
int smx_loudness_meter_flush(smx_loudness_meter *m);
int64_t smx_loudness_meter_position(const smx_loudness_meter *m);   /* samples per channel since reset */
int smx_loudness_meter_step_f32(smx_loudness_meter *m, const float *x, int64_t len, float *out);
int smx_loudness_meter_step_f64(smx_loudness_meter *m, const double *x, int64_t len, double *out);
int smx_loudness_meter_step_card_f32(smx_loudness_meter *m, void *stream, const float *d_x, int64_t len, int64_t x_stride, float *d_out);
int smx_loudness_meter_read_f32(smx_loudness_meter *m, int what, float *out);
int smx_loudness_meter_read_f64(smx_loudness_meter *m, int what, double *out);
int smx_loudness_meter_read_card_f32(smx_loudness_meter *m, void *stream, int what, float *d_out);

/* ---- Pcen: per-channel energy normalisation (Wang et al. 2017; Lostanlen et al. 2019; librosa.pcen with max_size = 1; the
 * reference has no such module) ----------------------------------------------------------------------------------------------
 * S is [rows; frames], non-negative and finite, frames fastest; a row is one (leading index, band).  Float64 inside, every
 * product, quotient and sum rounded on its own (no fused operation), one rounding to the dtype of the input:
 *     u[t] = scale * (double)S[t]
 *     M[t] = a * M[t-1] + s * u[t]          the two products, then the sum; M[-1] = zi[row], or u[0] when zi is NULL
 *     sm   = exp(-gain * (log(eps) + log1p(M[t] / eps)))
 *     out  = log1p(u * sm / bias)                                   power == 0
 *          = exp(power * (log(u) + log(sm))), 0 where u == 0        bias == 0
 *          = bias^power * expm1(power * log1p(u * sm / bias))       otherwise
 * s, a = 1.0 - s, log(eps) and bias^power are computed once on the host in float64.  Time is not cut into blocks: both kernels
 * (SMX_DISABLE_FAST=1 forces the general one), a leading slice of a batch, a call continued from another call's zf and every
 * chunking of the stream kernel give the same bits.  Negative or non-finite cells do not fault and are not otherwise specified.
 *
 *   smx_pcen_create      s = b when has_b; otherwise T = time_constant * sr / hop and s = (sqrt(1 + 4 T T) - 1) / (2 T T).
 *                        Refused in words: gain < 0, bias < 0, power < 0, eps <= 0, time_constant <= 0, sr or hop <= 0,
 *                        b outside [0, 1], scale <= 0, power == 0 together with bias == 0, any non-finite parameter.
 *   smx_pcen_coefficient s.
 *   smx_pcen_tile_min_frames  calls of at least this many frames (16) take the tile kernel, shorter ones the general kernel.
 *   smx_pcen_apply_*     [rows; frames] -> [rows; frames]; zi: NULL or [rows] float64; zf: NULL or [rows] float64, M at the
 *                        last frame.  frames = 0 hands zi back as zf (zero without one).
 *   smx_pcen_smooth_*    the smoother alone: M rounded once to the dtype of S.
 *   smx_pcen_of_audio_*  audio [lead; n] -> [lead; n_mels; frames]: smx_pcen_apply_* of smx_mel_spectrogram_* with power 1.0,
 *                        bit for bit; the mel spectrogram lies in device scratch and never leaves the device.
 *   smx_pcen_kernel_*    Pcen.Kernel.{prepare, step, flush, reset}: one double per row stays on the device (M at the last frame
 *                        fed); whether the stream has started is a host flag.  A step takes [rows; m] and returns [rows; m]
 *                        (latency zero); the first non-empty step takes M[-1] from its own first column.  The concatenated
 *                        steps equal smx_pcen_apply_* of the whole spectrogram bit for bit.  flush emits nothing and drains the
 *                        kernel: a step after it is refused until reset.  The first step allocates the state on its device;
 *                        the state is input and output of every later step, so a kernel belongs to that device (another is
 *                        refused in words) and to one stream at a time: steps on different streams are the caller's to order.
 *
 * The device-resident forms end in `_card_f32` and take the stream directly after the first argument (tables and laws of their
 * own: tests/test_gpu_placement_pcen.py, tests/test_gpu_streams_pcen.py).  Rows of d_x lie x_stride >= frames (of_audio: >= n)
 * elements apart and may start at any 4-byte position, results are dense; d_zi and d_zf are DEVICE arrays here and may be the
 * same array.  Everything is enqueued on `stream`; nothing synchronises it. */
typedef struct smx_pcen smx_pcen;
typedef struct smx_pcen_kernel smx_pcen_kernel;
int smx_pcen_create(int64_t sr, int64_t hop, double gain, double bias, double power, double time_constant, double eps, int has_b,
                    double b, double scale, smx_pcen **out);
void smx_pcen_destroy(smx_pcen *c);
double smx_pcen_coefficient(const smx_pcen *c);
int64_t smx_pcen_tile_min_frames(void);
int smx_pcen_apply_f32(const smx_pcen *c, const float *x, int64_t rows, int64_t frames, const double *zi, float *out, double *zf);
int smx_pcen_apply_f64(const smx_pcen *c, const double *x, int64_t rows, int64_t frames, const double *zi, double *out, double *zf);
int smx_pcen_apply_card_f32(const smx_pcen *c, void *stream, const float *d_x, int64_t rows, int64_t frames, int64_t x_stride,
                            const double *d_zi, float *d_out, double *d_zf);
int smx_pcen_smooth_f32(const smx_pcen *c, const float *x, int64_t rows, int64_t frames, const double *zi, float *out);
int smx_pcen_smooth_f64(const smx_pcen *c, const double *x, int64_t rows, int64_t frames, const double *zi, double *out);
int smx_pcen_smooth_card_f32(const smx_pcen *c, void *stream, const float *d_x, int64_t rows, int64_t frames, int64_t x_stride,
                             const double *d_zi, float *d_out);
int smx_pcen_of_audio_f32(const smx_pcen *c, const smx_stft_config *sc, const smx_mel_config *mc, const float *x, int64_t lead,
                          int64_t n, float *out);
int smx_pcen_of_audio_f64(const smx_pcen *c, const smx_stft_config *sc, const smx_mel_config *mc, const double *x, int64_t lead,
                          int64_t n, double *out);
int smx_pcen_of_audio_card_f32(const smx_pcen *c, void *stream, const smx_stft_config *sc, const smx_mel_config *mc,
                               const float *d_x, int64_t lead, int64_t n, int64_t x_stride, float *d_out);
int smx_pcen_kernel_prepare(const smx_pcen *c, int64_t rows, smx_pcen_kernel **out);
void smx_pcen_kernel_destroy(smx_pcen_kernel *k);
int smx_pcen_kernel_reset(smx_pcen_kernel *k);
int smx_pcen_kernel_flush(smx_pcen_kernel *k);
int smx_pcen_kernel_step_f32(smx_pcen_kernel *k, const float *x, int64_t m, float *out);
int smx_pcen_kernel_step_f64(smx_pcen_kernel *k, const double *x, int64_t m, double *out);
int smx_pcen_kernel_step_card_f32(smx_pcen_kernel *k, void *stream, const float *d_x, int64_t m, int64_t x_stride, float *d_out);

#ifdef __cplusplus
}
#endif
#endif /* SOUNDML_AMD_H */
