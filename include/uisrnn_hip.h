/*
 * uisrnn_hip.h -- C ABI of the MI355X (gfx950) UIS-RNN beam-search decoder.
 *
 * This is the drop-in boundary for ONE path of google/uis-rnn: the inference
 * beam search  UISRNN.predict -> predict_single -> _calculate_score ->
 * _update_beam_state -> CoreRNN / BeamState
 * (reference: uisrnn/uisrnn.py:388-590, uisrnn/loss_func.py:19-41).
 *
 * The reference has no FFI of its own -- its boundary is the Python method set
 * on uisrnn.UISRNN (uisrnn/__init__.py:26-30).  A maintainer binds these entry
 * points with ctypes (cffi is the other option) exactly as uisrnn_amd/_capi.py
 * does; INTEGRATION.md shows the stub.  Plain C types only: no torch, no HIP
 * types in the signatures.  Device pointers are passed as void* / float*.
 *
 * Threading: a handle is bound to one HIP device and is not thread-safe; use
 * one handle per thread / per rank.  All calls are blocking.
 * Errors: every function returns UIS_OK (0) or a negative uis_status;
 * uis_last_error() returns a thread-local message for the last failure; the
 * pointer is good until this thread's next failing call (copy the text if it
 * is to be kept, and call it AFTER the call it explains -- as an argument of
 * the same printf its evaluation order is unspecified in C).
 */
#ifndef UISRNN_HIP_H_
#define UISRNN_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UIS_ABI_VERSION 6

typedef enum uis_status {
  UIS_OK = 0,
  UIS_ERR_INVALID_ARG = -1,   /* NULL pointer, non-positive size, bad option      */
  UIS_ERR_DIM_MISMATCH = -2,  /* maps to the reference's ValueError (uisrnn.py:518-521) */
  UIS_ERR_NO_DEVICE = -3,     /* no usable gfx950 device / HIP runtime failure at create */
  UIS_ERR_HIP = -4,           /* a HIP call failed during decode                   */
  UIS_ERR_OOM = -5,           /* device or host allocation failed                  */
  UIS_ERR_CLUSTER_CAP = -6,   /* a surviving hypothesis needed more than max_clusters
                                 clusters; labels_out of the flagged utterances are
                                 invalid -- retry with a larger cap (the Python host does) */
  UIS_ERR_UNSUPPORTED = -7    /* an option value beyond a field width (beam_size > 32767, look_ahead > 1024,
                                 max_clusters > 4096), a UIS_FLAG_RESIDENT request where no one-launch kernel
                                 applies; also: a look_ahead >= 2 window had more live assignment prefixes than
                                 the level capacity (uis_decode_opts.level_cap: bit 1 of the utterance's flags in
                                 uis_last_decode_info; decode those again with a larger one -- a larger
                                 max_clusters cannot help)                                    */
} uis_status;

/*
 * Model parameters consumed by predict (reference: UISRNN.__init__ / load,
 * uisrnn/uisrnn.py:83-107,149-170; CoreRNN, uisrnn/uisrnn.py:32-52).
 * All arrays are host pointers, float32, row-major, PyTorch layouts; they are
 * copied at uis_create and need not outlive it.
 */
typedef struct uis_model_desc {
  int32_t observation_dim;            /* D  (args.observation_dim)            */
  int32_t rnn_hidden_size;            /* H  (args.rnn_hidden_size)            */
  int32_t rnn_depth;                  /* number of GRU layers                 */
  int32_t reserved0;
  const float* const* gru_weight_ih;  /* [depth] -> (3H, D) layer 0, (3H, H) above; gates r|z|n */
  const float* const* gru_weight_hh;  /* [depth] -> (3H, H)                   */
  const float* const* gru_bias_ih;    /* [depth] -> (3H)                      */
  const float* const* gru_bias_hh;    /* [depth] -> (3H)                      */
  const float* linear_mean1_weight;   /* (H, H)                               */
  const float* linear_mean1_bias;     /* (H)                                  */
  const float* linear_mean2_weight;   /* (D, H)                               */
  const float* linear_mean2_bias;     /* (D)                                  */
  const float* rnn_init_hidden;       /* (depth, H)  (rnn_init_hidden[:,0,:]) */
  const float* sigma2;                /* (D)                                  */
  double transition_bias;             /* p0 in (0,1)                          */
  double crp_alpha;                   /* alpha > 0                            */
} uis_model_desc;

/* Inference options (reference: uisrnn/arguments.py:172-193). */
typedef struct uis_decode_opts {
  int32_t beam_size;       /* args.beam_size       (>= 1; beyond 256 -- and wherever max_clusters outgrows the
                              select kernels' LDS -- the window machinery decodes: a launch per sub-step,
                              candidate lists in HBM; at most 32767)                                */
  int32_t look_ahead;      /* args.look_ahead      (>= 1, at most 1024)       */
  int32_t test_iteration;  /* args.test_iteration  (>= 1)                     */
  int32_t max_clusters;    /* per-hypothesis cluster cap; 0 = default (16)    */
  uint32_t flags;          /* UIS_FLAG_*                                      */
  int32_t n_streams;       /* utterance groups decoded concurrently, each on its
                              own HIP stream; 0 = default (1), at most 8       */
  int32_t level_cap;       /* look_ahead >= 2: hypotheses an intermediate level of a window may hold per
                              utterance; 0 = default (32768), at most 524287.  A window with more live
                              assignment prefixes sets bit 1 of the utterance's flags and the call returns
                              UIS_ERR_UNSUPPORTED: decode those utterances again with a larger level_cap
                              (the Python host does, until the device's memory says UIS_ERR_OOM)      */
  int32_t reserved[1];
} uis_decode_opts;

#define UIS_FLAG_NO_DEDUP   0x1u /* run one RNN row per surviving hypothesis even when
                                    several share the same cluster state (A/B switch;
                                    results are bit-identical either way)            */
#define UIS_FLAG_GRAPH      0x2u /* replay the per-step kernels from a captured hipGraph
                                    (32 steps per graph) instead of launching eagerly  */
#define UIS_FLAG_GENERIC_SELECT 0x8u /* use the general score/prune kernel even where the
                                    wave-synchronous fast path applies (A/B switch;
                                    results are bit-identical either way)            */
#define UIS_FLAG_RESIDENT   0x40u /* REQUIRE the one-launch decode (k_decode_resident: one workgroup
                                    per CU in clusters of 32 -- one cluster per XCD -- W_hh in
                                    registers and the mean-head tiles in LDS for the whole decode,
                                    one XCD per utterance subset, in-launch XCD barriers between
                                    the stages of a step; launched cooperatively so that all
                                    workgroups are co-resident) and fail with UIS_ERR_UNSUPPORTED
                                    where it does not apply.  It is the DEFAULT wherever it
                                    applies: look_ahead 1, rnn_depth 1, rnn_hidden_size 65 .. 256 or
                                    385 .. 512 and observation_dim up to 256 or 385 .. 512 (the model is
                                    padded up to 128 / 256 / 512 x 128 / 256 / 512 at uis_create; rnn_depth >= 2
                                    at those sizes: k_decode_deep, UIS_DK_DEEP),
                                    beam_size * (max_clusters + 1) <= 256, one stream, a device
                                    whose CU count is a multiple of 32; small models (hidden size up
                                    to about 64, any rnn_depth) with one workgroup per utterance;
                                    look_ahead >= 2 at rnn_depth 1 and those hidden sizes with the
                                    window's sub-step as the select stage (UIS_DK_WINDOW)        */
#define UIS_FLAG_STEPWISE   0x80u /* keep the launch-per-step path (four kernels per decode
                                    step) even where the one-launch decode applies (A/B switch;
                                    results are bit-identical either way)                     */
#define UIS_FLAG_SMALL_TILES 0x200u /* keep the split-K dense stages even where the wave-per-row-tile
                                    ones apply: the big-tile kernels of the launch-per-step path
                                    (thousands of rnn rows per step) and k_decode_big of the one-launch
                                    path (more utterances than workgroups); A/B switch, results are
                                    bit-identical either way                                     */
#define UIS_FLAG_PERSISTENT 0x400u /* uis_stream_begin only: the one-launch decode kernel STAYS on the device
                                    between pushes and takes pushes / label requests from a mailbox in
                                    host-coherent pinned memory -- a push costs no launch and no copy
                                    engine, only the steps themselves.  The kernel occupies every compute
                                    unit until uis_stream_end or until it has been idle for
                                    UIS_PERSIST_IDLE_MS (environment, default 50 ms; it then leaves and
                                    the next push starts a new one).  Needs the one-launch shape, at
                                    most one utterance per compute unit, unpadded observation_dim;
                                    pushes of more than 16 frames per utterance go the ordinary way */
#define UIS_FLAG_OWNER_SELECT 0x800u /* one-launch decode: keep the select of an utterance on ONE
                                    workgroup (k_decode_resident) even where the replicated select
                                    applies (k_decode_rs: at most 8 utterances per XCD, every
                                    workgroup of the XCD decides all of them, one wave each -- one
                                    in-launch hand-off less per step and a select short enough for a
                                    single wave); A/B switch, results are bit-identical either way */
#define UIS_FLAG_REPLICATED_SELECT 0x1000u /* accepted and ignored: the bit is reserved.  It once selected k_decode_rs's
                                    "wide" class (beam_size 17 .. 32, observation_dim 512) and its two-utterances-
                                    per-wave class where they were not the default; both measured slower than the
                                    owner-select kernel and were removed; a decode with the flag runs exactly as one
                                    without it                                                                  */
#define UIS_FLAG_CLUSTER_BARRIERS 0x8000u /* one-launch decode with the owner select (k_decode_resident): keep the
                                    cluster-wide barriers between GRU, linear_mean1 and linear_mean2 instead of
                                    the per-producer phase words (a consumer wave waits for the four workgroups
                                    that produce its K-slice); A/B switch, results are bit-identical either way */
#define UIS_FLAG_COHORTS 0x10000u /* accepted and ignored: the bit is reserved.  It once selected k_decode_coh (two utterance
                                    cohorts in flight per XCD), which measured slower than k_decode_big<WS> and was removed;
                                    a decode with the flag runs exactly as one without it                               */
#define UIS_FLAG_AGENT_FLAGS 0x20000u /* one-launch decode: publish the per-producer phase words of the dense-stage hand-offs
                                    with an AGENT-scope store (`global_store sc1`: the HIP memory model's by-the-book form for
                                    a word other workgroups read) instead of the workgroup-scope store that stays in the
                                    XCD's L2 (uis_kernels.hip: rs_flag_publish).  A run-time choice in one binary since round
                                    6 (the environment's UIS_AGENT_FLAGS=1 does the same); bit-identical; its cost is on
                                    record: profiles/r06_agent_flags_ab.txt -- it is NOT small, hence opt-in          */
#define UIS_FLAG_DEBUG_SCORES 0x2000u /* test hook: keep every candidate score of every window (step) --
                                    the arrays _calculate_score returns (uisrnn/uisrnn.py:455-477) -- for
                                    uis_debug_scores(); costs device memory and one store per candidate */
#define UIS_FLAG_TEST_MISPLACED 0x100u /* test hook: one workgroup of the one-launch decode reports
                                    a wrong XCD, as if the (observed, not promised) workgroup
                                    placement had changed.  The call must then fall back to the
                                    launch-per-step path by itself -- and stay there for this
                                    handle -- or, with UIS_FLAG_RESIDENT, fail with UIS_ERR_HIP */
#define UIS_FLAG_TEST_STALL 0x4000u /* test hook (k_decode_rs): one workgroup stops publishing its phase
                                    word after a few steps, as if it had died.  The waves that wait for
                                    it give up after ~1 s, the launch ends, and the call falls back to
                                    the launch-per-step path (with UIS_FLAG_RESIDENT: UIS_ERR_HIP) */
#define UIS_FLAG_PROFILE    0x4u /* launch every kernel with start/stop HIP events on the
                                    decode stream (hipExtLaunchKernelGGL: the dispatch's
                                    own begin/end timestamps) and fill uis_stats.kernel_* */

#define UIS_N_KERNELS 8
typedef struct uis_stats {
  int32_t n_steps;                    /* lock-step decode steps executed            */
  int32_t max_clusters_seen;          /* max clusters in any surviving hypothesis   */
  int64_t rnn_rows;                   /* RNN rows actually evaluated (after dedup)  */
  int64_t rnn_rows_nodedup;           /* rows without dedup = surviving hypotheses  */
  int64_t candidates;                 /* candidates scored                           */
  double  decode_ms;                  /* device time of the whole decode (events)   */
  double  kernel_ms[UIS_N_KERNELS];   /* UIS_FLAG_PROFILE: summed per kernel class  */
  int64_t kernel_launches[UIS_N_KERNELS];
  int32_t n_overflow;                 /* utterances that hit UIS_ERR_CLUSTER_CAP    */
  int32_t n_streams;                  /* utterance groups used                       */
  int32_t decode_kernel;              /* UIS_DK_*: the kernel family that ran the decode steps */
  int32_t decode_launches;            /* launches of the one-launch decode kernel in this decode: 1, or 2 and more (2 - 4 by
                                         the library's own slice schedule, up to 8 with UIS_SPLIT_FRAMES) when the list came
                                         from host memory and its later frames travelled behind the earlier launches
                                         (uis_decode / uis_decode_f64: k_decode_rs, k_decode_big<WS>, k_decode_resident with
                                         one utterance per workgroup; UIS_NO_SPLIT=1 keeps 1); 0 on the launch-per-step path */
} uis_stats;

/* uis_stats.decode_kernel: which kernels ran the decode steps (the dispatch rule lives in the
 * library, uis_decoder.hip: callers that want to NAME the kernel read it here) */
enum {
  UIS_DK_NONE = 0,
  UIS_DK_STEPWISE = 1,   /* launch per step: k_select* / k_window + the dense kernels below   */
  UIS_DK_RS = 2,         /* one launch, replicated single-wave select (k_decode_rs)           */
  UIS_DK_RESIDENT = 3,   /* one launch, owner select (k_decode_resident)                      */
  UIS_DK_BIG = 4,        /* one launch, a wave per row tile (k_decode_big)                    */
  UIS_DK_BIG_WS = 5,     /* ... with a rank's selects running concurrently (k_decode_big<WS>) */
  UIS_DK_SMALL = 6,      /* one launch, one workgroup per utterance: small models, any rnn_depth, any look_ahead (k_decode_small) */
  UIS_DK_WINDOW = 7,     /* one launch, look_ahead >= 2: a window sub-step as the select stage (k_decode_big<WIN>) */
  UIS_DK_DEEP = 8,       /* one launch, rnn_depth >= 2 at hidden size 128 / 256 / 512: the weight slot refilled per stage (k_decode_deep) */
  UIS_DK_BIG_COH = 9     /* reserved, never reported (was k_decode_coh, removed)                 */
};
/* ... in bits 16..23 for UIS_DK_RS its instantiation: 1 base, 2 base with the shape of BASELINE configs[1] as
 * compile-time constants; 3 .. 6 are reserved (never reported: 3 and 4 were the removed two-per-wave and wide
 * classes); and, in bits 8..15 for UIS_DK_STEPWISE, the dense kernels' family */
enum { UIS_DF_DENSE = 1 /* k_dense_* split-K */, UIS_DF_BIG = 2 /* k_big_* */, UIS_DF_WT = 3 /* k_wt_* */ };

/* kernel classes for uis_stats.kernel_ms */
enum {
  UIS_K_INPUT_PROJ = 0, /* W_ih0 x + b over all frames, new-cluster MSE      */
  UIS_K_SELECT = 1,     /* score + prune + commit                           */
  UIS_K_GRU = 2,        /* hidden-side GRU GEMM + gates                     */
  UIS_K_HEAD1 = 3,      /* linear_mean1 + relu                              */
  UIS_K_HEAD2 = 4,      /* linear_mean2 + running-mean update               */
  UIS_K_BACKTRACE = 5,  /* back-pointer walk -> labels                      */
  UIS_K_UPPER_IN = 6,   /* input-side GEMM of GRU layers >= 1               */
  UIS_K_EXPAND = 7      /* look_ahead >= 2: intermediate sub-step expansion */
};

typedef struct uis_handle uis_handle;

int32_t uis_abi_version(void);

/* UIS_NUMERICS_VERSION of include/uis_numerics.h this library was built with. */
int32_t uis_numerics_version(void);

/* What this binary was built with: a mask of UIS_BUILD_* (none is defined at present: always 0). */
#define UIS_BUILD_COHORTS 0x1u  /* reserved, never set (was: k_decode_coh compiled in) */
uint32_t uis_build_flags(void);

/* Number of visible HIP devices (0 if none / runtime unusable). */
int32_t uis_device_count(void);

/*
 * Create a decoder on HIP device `device`: uploads the weights in the padded
 * layouts the kernels use and precomputes the per-model constants
 * (m0, h1) = CoreRNN(0, rnn_init_hidden)  (uisrnn/uisrnn.py:435-439) and
 * w = 1 / (2 sigma2)  (uisrnn/uisrnn.py:414).
 */
int32_t uis_create(const uis_model_desc* desc, int32_t device, uis_handle** out);

void uis_destroy(uis_handle* h);

/*
 * Decode n_utt utterances (reference: UISRNN.predict over a list,
 * uisrnn/uisrnn.py:564-590; each one UISRNN.predict_single, :479-562).
 *   frames   : host, float32, [offsets[n_utt], D] row-major (utterance u owns rows
 *              offsets[u] .. offsets[u+1]); the caller has already cast the
 *              reference's float64 input to float32 (uisrnn.py:525-526)
 *   offsets  : host, int64, [n_utt + 1], offsets[0] == 0, non-decreasing
 *   labels_out : host, int32, [offsets[n_utt]]  -- predicted cluster id per frame
 *              (trace[-N:] of the best hypothesis, uisrnn.py:561)
 *   scores_out : host, float32, [n_utt] or NULL -- neg_likelihood of the best hypothesis
 *   stats    : optional
 * Empty utterances (N == 0) are allowed and produce no labels.
 * The frames travel to the device inside the call; where the one-launch kernels apply and the utterances are
 * equally long, the decode runs as a few launches with the later frames of every utterance copied and
 * projected behind the earlier launches (uis_stats.decode_launches; identical results).
 */
int32_t uis_decode(uis_handle* h, const float* frames, const int64_t* offsets,
                   int32_t n_utt, const uis_decode_opts* opts,
                   int32_t* labels_out, float* scores_out, uis_stats* stats);

/*
 * Same, taking the utterances the way the reference's predict() receives them
 * (uisrnn/uisrnn.py:564-590: a list of [N_u, D] float64 arrays, dtype checked at
 * :511-513) -- no packed float32 copy on the caller's side:
 *   utterances : host, [n_utt] pointers, utterances[u] -> float64 [n_frames[u], D]
 *                row-major, contiguous (may be NULL where n_frames[u] == 0)
 *   n_frames   : host, int64, [n_utt]
 * The cast to float32 (round to nearest even, what torch's .float() does at
 * :524-526) is done by the library: a few host threads fill a pinned staging
 * buffer chunk by chunk, each chunk's copy to the device and input projection
 * running while the next chunk is cast.  labels_out covers sum(n_frames) frames
 * in utterance order.
 */
int32_t uis_decode_f64(uis_handle* h, const double* const* utterances, const int64_t* n_frames,
                       int32_t n_utt, const uis_decode_opts* opts,
                       int32_t* labels_out, float* scores_out, uis_stats* stats);

/*
 * Same, with frames / labels_out / scores_out resident on the handle's device
 * (HBM pointers, e.g. torch tensor data_ptr()); offsets stays on the host.
 * No PCIe transfer of the frame stream happens inside the call.
 */
int32_t uis_decode_device(uis_handle* h, const float* d_frames, const int64_t* offsets,
                          int32_t n_utt, const uis_decode_opts* opts,
                          int32_t* d_labels_out, float* d_scores_out, uis_stats* stats);

/*
 * Device tensors in: decode and push straight from what a speaker encoder left in HBM.
 *
 * A uis_tensor describes one block of rows on the handle's device: `rows` rows of observation_dim elements of `dtype`,
 * the inner dimension contiguous, row r at data + r * row_stride elements (row_stride >= observation_dim: a slice of a
 * padded [U, T, D] batch, a [:, :D] view of a wider tensor, any base alignment).  One kernel launch (k_ingest,
 * csrc/uis_ingest.hip) gathers the blocks of a call, in list order, into the packed float32 [F, D] stream the other
 * entry points receive, converting on the way:
 *   float64 -> float32  round to nearest even, bit for bit the cast of uis_decode_f64 (and numpy's astype(float32)):
 *                       results that are float32 subnormals and values that overflow to +-inf included
 *   float16, bfloat16   exact, subnormal inputs included
 * Everything behind the packed stream is what it was, so a call here gives the bits of its host sibling on the same
 * values.
 *
 * producer_stream: the HIP stream on which the tensors were written (a hipStream_t, e.g. torch's
 * torch.cuda.current_stream().cuda_stream), NULL for the default stream.  The call records an event there and its own
 * stream waits for it before the first read: no synchronisation is needed on the caller's side.  The calls block as
 * their siblings do: outputs are complete, and the tensors free to be rewritten, on return.
 *
 * Checked on the host before any GPU work (UIS_ERR_INVALID_ARG): data NULL with rows > 0, rows < 0, an unknown dtype,
 * row_stride < observation_dim with rows > 0, data not aligned to its element size, capacity_rows below the rows given.
 *
 *   uis_ingest_tensors        the kernel alone: n blocks -> d_frames_out, float32 [sum rows, D] on the device, with room
 *                             for capacity_rows rows
 *   uis_tensors_decode        uis_decode_device of the utterances given as one block each (rows 0: an empty utterance):
 *                             the blocks are gathered into the handle's own frame buffer and decoded from there.
 *                             d_labels_out / d_scores_out on the device, as there; the per-call tables (uis_decode_limits,
 *                             uis_frame_bias, uis_frame_speakers, uis_min_turn) belong to it as to every decode, and the
 *                             uis_last_decode_* readouts are valid after it
 *   uis_tensors_stream_push   uis_stream_push with utterance u's new frames in chunks[u] (rows 0: none): the same checks
 *                             in the same order, a pending uis_frame_bias / uis_stream_speakers table applies as there;
 *                             the frames never leave the device.  A UIS_FLAG_PERSISTENT session returns
 *                             UIS_ERR_UNSUPPORTED before touching anything (its frames would have to travel through the
 *                             host mailbox) and stays usable and unchanged
 * (The latter two are named tensors-first: the prefixes uis_decode / uis_stream_ are enumerated by the call-table test.)
 */
enum { UIS_DTYPE_F32 = 0, UIS_DTYPE_F64 = 1, UIS_DTYPE_F16 = 2, UIS_DTYPE_BF16 = 3 };
typedef struct uis_tensor {
  const void* data;    /* device pointer to the first row (may be NULL where rows == 0) */
  int64_t rows;
  int64_t row_stride;  /* elements between two rows, >= observation_dim */
  int32_t dtype;       /* UIS_DTYPE_* */
  int32_t reserved;    /* 0 */
} uis_tensor;
int32_t uis_ingest_tensors(uis_handle* h, const uis_tensor* blocks, int32_t n, void* producer_stream,
                           float* d_frames_out, int64_t capacity_rows);
int32_t uis_tensors_decode(uis_handle* h, const uis_tensor* utterances, int32_t n_utt, void* producer_stream,
                           const uis_decode_opts* opts, int32_t* d_labels_out, float* d_scores_out, uis_stats* stats);
int32_t uis_tensors_stream_push(uis_handle* h, const uis_tensor* chunks /* [n_utt of the session] */,
                                void* producer_stream);

/*
 * After a decode: per-utterance overflow flags (1 = hit the cluster cap) and
 * the full final beam scores, for the host-side retry loop and the parity tests.
 *   overflow_out : host int32 [n_utt] or NULL
 *   beam_scores_out : host float32 [n_utt * beam_size] or NULL (+inf padded)
 */
int32_t uis_last_decode_info(uis_handle* h, int32_t* overflow_out, float* beam_scores_out);

/*
 * The sizes uis_last_decode_info copies with: n_utt and beam_size of this handle's last
 * uis_decode* call (0 / 0 when that call was refused before it started, e.g. UIS_ERR_UNSUPPORTED
 * for its options -- a caller must size its buffers from here, not from what it asked for).
 */
int32_t uis_last_decode_shape(uis_handle* h, int32_t* n_utt_out, int32_t* beam_size_out);

/*
 * Which kernel instantiation ran: the entry of the library's kernel tables behind this handle's last uis_decode*
 * call, or behind the last launch of a uis_stream_push of the open session (a UIS_FLAG_PERSISTENT session: the
 * launch that stays, however many pushes it has served), as the table lookup itself returned it:
 *   out[0] family  : UIS_DK_*
 *   out[1], out[2] : the instantiation's hidden size and observation dim (the model's, padded: 128 / 256 / 512)
 *   out[3] variant : the compile-time shape class (0 generic, 1 beam 10 / cap 16, 2 beam 20 / cap 11, 3 beam 50 /
 *                    cap 12 / look_ahead 2); for UIS_DK_RS its kind (bits 16..23 of uis_stats.decode_kernel); for
 *                    UIS_DK_DEEP 1 = the look_ahead >= 2 kernel
 *   out[4] persist : 1 = the kernel a UIS_FLAG_PERSISTENT session keeps on the device
 * UIS_DK_SMALL and UIS_DK_STEPWISE have no table: their family with the model's padded sizes, variant 0.  All zero
 * after a decode that was refused before it chose a kernel.
 */
int32_t uis_last_decode_instantiation(uis_handle* h, int32_t out[5]);

/*
 * The kernel tables themselves, a row of five int32 (as above) per instantiation: fills at most `cap` rows of
 * `rows` (may be NULL) and returns the number of rows there are.  Needs no device.
 */
int32_t uis_decode_kernel_table(int32_t* rows, int32_t cap);

/*
 * After a decode with UIS_FLAG_DEBUG_SCORES: the candidate scores of every window (look_ahead 1: of
 * every decode step),
 *   scores_out[(((w * n_utt + u) * beam_size + b) * C + c_1) * C ... + c_L],   C = max_clusters + 1
 * = what _calculate_score (uisrnn/uisrnn.py:455-477) returns for hypothesis b of utterance u in
 * window w (0 .. ceil(test_iteration * longest utterance / look_ahead) - 1) for the assignment
 * tuple (c_1 .. c_L), +inf where the reference's padded score_set (uisrnn.py:534-545) holds +inf:
 * clusters past K_b, hypotheses past the live beam, windows past the utterance's end, tuples
 * through a non-finite prefix.  A ragged last window of Lw < L frames has its scores at index 0 of
 * the missing dimensions.  `capacity` = floats available at scores_out; returns
 * UIS_ERR_INVALID_ARG when the last decode kept none or the buffer is too small.
 */
int32_t uis_debug_scores(uis_handle* h, float* scores_out, int64_t capacity);

/*
 * Read back the per-model constants computed at uis_create with the decode
 * kernels: m0 [D] and h1 [depth * H], (m0, h1) = CoreRNN(0, rnn_init_hidden)
 * (uisrnn/uisrnn.py:435-439).  Host pointers; either may be NULL.
 */
int32_t uis_model_constants(uis_handle* h, float* m0_out, float* h1_out);

/*
 * One CoreRNN.forward for seq_len = 1, batch = 1 (uisrnn/uisrnn.py:45-52) through the
 * decode kernels: x [D], h_in [depth * H] -> mean_out [D], h_out [depth * H] (host
 * pointers).  Unit-level entry point for parity tests; the decode does not call it.
 */
int32_t uis_rnn_step(uis_handle* h, const float* x, const float* h_in, float* mean_out, float* h_out);

/*
 * Online decoding (the caller side of the path: UIS-RNN is an online model; the reference
 * only offers offline predict(), uisrnn/uisrnn.py:479-590, with the test_iteration replay).
 * A session keeps the beam, the cluster states and the back-pointers of n_utt utterances on
 * the device.  Semantics = predict_single with test_iteration 1 and look_ahead 1: whatever the
 * chunking, the labels and scores equal those of one uis_decode over the whole utterances
 * (bit for bit).  One session per handle; uis_decode is refused while it is open.
 *
 *   uis_stream_begin  opts->test_iteration and look_ahead must be 1; max_frames = the most frames
 *                     any utterance will receive in this session (4 * beam_size bytes each) -- with
 *                     uis_stream_commit (below): the most it holds between two commits.
 *                     opts->flags: UIS_FLAG_PERSISTENT keeps the decode kernel on the device
 *                     between pushes (lowest latency, occupies the whole device; UIS_ERR_UNSUPPORTED
 *                     where the session's shape does not allow it)
 *   uis_stream_push   frames: host float32, the new frames of utterance 0, then 1, ...;
 *                     counts[u] >= 0 = how many of them belong to utterance u (0 is fine)
 *   uis_stream_labels labels_out: host int32, for every utterance all frames received so far
 *                     (packed in utterance order) under the currently best hypothesis -- earlier
 *                     labels may still change with later frames, as in any beam search;
 *                     scores_out [n_utt] / overflow_out [n_utt] or NULL.  Returns
 *                     UIS_ERR_CLUSTER_CAP (labels still written) if a cap was hit.
 *   uis_stream_end    frees the session
 */
int32_t uis_stream_begin(uis_handle* h, int32_t n_utt, const uis_decode_opts* opts, int64_t max_frames);
int32_t uis_stream_push(uis_handle* h, const float* frames, const int32_t* counts);
int32_t uis_stream_labels(uis_handle* h, int32_t* labels_out, float* scores_out, int32_t* overflow_out);
int32_t uis_stream_end(uis_handle* h);

/*
 * max_speakers: decode under a per-utterance bound on the clusters a hypothesis holds.
 *
 * limit[u] >= 1 is the bound of utterance u, 0 means no bound.  The rule: a hypothesis that already holds
 * K >= limit[u] clusters has no new-cluster candidate -- what the reference's beam search would do if
 * _calculate_score gave +inf to the new-cluster entry of such a state.  Nothing else changes: the candidates of the
 * existing clusters, their priors (the denominators still contain crp_alpha), the float32 accumulation, the prune
 * order and the tie rules are the unbounded decode's, and a bound that never binds gives its bits.  K is the
 * hypothesis' cluster count whatever produced it: across test_iteration repetitions, inside a look-ahead window (the
 * K of the prefix being extended), after uis_stream_prime / _import / _retire.  A hypothesis whose K is already above
 * the bound (a primed prefix, an imported blob, a lowered limit) is kept: it opens nothing more.  After a retirement
 * K drops and clusters may open again: the bound is on the clusters held at once, not on the ids ever handed out.
 * A hypothesis bounded by N <= max_clusters never sets the overflow word.
 *
 *   uis_decode_limits      limits: host int32 [n_utt], each in [0, 4096] (else UIS_ERR_INVALID_ARG and the pending
 *                          table is left as it was); NULL clears a pending table.  The table belongs to the NEXT
 *                          uis_decode / uis_decode_f64 / uis_decode_device / uis_stream_begin on this handle, which
 *                          consumes it whether it succeeds or not and must have exactly n_utt utterances (else that
 *                          call returns UIS_ERR_INVALID_ARG and nothing runs).  A decode without a pending table
 *                          is unbounded, whatever an earlier call used.
 *   uis_stream_limits      limits: host int32 [n_utt of the session]: replaces the open session's table between two
 *                          pushes, all or nothing.  The limits belong to the session's slots, not to the streams in
 *                          them: uis_stream_restart keeps them, an imported utterance decodes on under the target
 *                          slot's limit, and blobs do not carry them.  (A UIS_FLAG_PERSISTENT session's resident
 *                          launch leaves the device for the call, as for the other session calls.)
 *   uis_stream_get_limits  out: host int32 [n_utt]: the session's table as given (0: no bound)
 *
 * uis_score_labels / uis_score_speakers score given labels and know no limits; the n-best, posterior and commit
 * readouts read what the decode left.
 */
int32_t uis_decode_limits(uis_handle* h, const int32_t* limits, int32_t n_utt);
int32_t uis_stream_limits(uis_handle* h, const int32_t* limits);
int32_t uis_stream_get_limits(uis_handle* h, int32_t* out);

/*
 * Per-frame transition_bias: decode (and score) under soft and hard turn priors.
 *
 * bias[t] in [0, 1] is the probability that frame t of the NEXT call that takes frames changes speaker -- the model's
 * scalar transition_bias made time-varying (a speaker-change detector's output, a segment boundary, the inside of a
 * word); NaN means "the model's own".  For every frame the library forms, in float64 with the C library's log and the
 * expressions of uis_create, (log(1 - b), log(b), log(b) + log(crp_alpha)); the step that decides frame t reads them
 * wherever it reads the model's three words today: a look_ahead-1 step, sub-step j of a look-ahead window (its own
 * frame), the second pass of test_iteration 2 (frame t % n).  Nothing else changes -- the ddCRP terms, the float32
 * accumulation, the prune order, the tie rules, max_speakers -- and an all-NaN table, or one holding exactly the model's
 * value, gives the decode without a table bit for bit.
 *
 * log(0) = -inf makes a candidate's loss +inf, and every select drops such a candidate: b = 0 keeps the frame with the
 * previous speaker (only the candidate of the last label is finite), b = 1 makes it change.  A contradiction -- b = 1 under
 * max_speakers 1, or b = 0 at a frame no hypothesis has a previous label for -- leaves an empty beam, reported as ever
 * (labels -1, score +inf).
 *
 *   uis_frame_bias   bias: host float64 [n_frames], each in [0, 1] or NaN (else UIS_ERR_INVALID_ARG, and the pending
 *                    table stays as it was); bias == NULL or n_frames == 0 clears a pending table.  The table belongs
 *                    to the NEXT uis_decode / uis_decode_f64 / uis_decode_device / uis_stream_push / uis_score_labels /
 *                    uis_score_speakers on this handle, in that call's frame order (utterance-major; a push: the
 *                    chunk's), and must hold exactly that call's frame count (else that call returns
 *                    UIS_ERR_INVALID_ARG and nothing runs).  The call consumes it whether it succeeds or not; a call
 *                    without a pending table uses the model's value, whatever an earlier call used.
 *
 * uis_stream_prime (its prefix is scored with the model's value) and a push into a UIS_FLAG_PERSISTENT session (whose
 * resident launch would need the table through its mailbox) refuse a pending table with UIS_ERR_UNSUPPORTED, consume it
 * and stay usable.  A decode with a table runs the kernels with the owner-side selects: where the decode without one
 * reports k_decode_rs or k_decode_big<WS>, uis_last_decode_instantiation reports k_decode_resident or k_decode_big.
 */
int32_t uis_frame_bias(uis_handle* h, const double* bias, int64_t n_frames);

/*
 * Known speakers: decode under partial speaker labels.
 *
 * tags[t] names who speaks at frame t of the NEXT decode: 0 = unknown, 1 .. 127 = a known speaker (a corrected segment,
 * an enrolled voice, a channel or ASR speaker tag; two snippets known to be the same person carry the same tag, two known
 * to differ carry different ones).  Every hypothesis holds a partial, injective binding of tags to its clusters.  At a
 * frame with tag g > 0, a hypothesis with K clusters has these candidates: if g is bound to cluster c*, only c*;
 * otherwise the clusters c < K that carry no tag, and the new cluster K (still subject to max_speakers) -- and the
 * candidate that wins binds g to its cluster.  At a frame with tag 0 every candidate is as without a table, clusters
 * that carry a tag included, and nothing is bound.  The same rule holds for sub-step j of a look-ahead window (its own
 * frame's tag, the binding of the prefix it extends) and for the later passes of test_iteration >= 2 (the tag of frame
 * t % n; bindings persist).  Nothing else changes -- the priors, the ddCRP terms, the float32 accumulation, the prune
 * order, the tie rules, max_speakers, uis_frame_bias -- and an all-zero table gives the decode without one bit for bit.
 *
 * A disallowed candidate has a loss of +inf, which every select drops.  A contradiction -- two tags under
 * max_speakers 1, a bias of 0 at a frame whose tag is bound to another cluster -- leaves an empty beam, reported as
 * ever (labels -1, score +inf).  Returned labels stay first-appearance integers: frames with equal tags get equal labels,
 * frames with different tags different ones.
 *
 *   uis_frame_speakers   tags: host uint8 [n_frames], each in 0 .. 127 (a larger value: UIS_ERR_INVALID_ARG, and the
 *                        pending table stays as it was); tags == NULL or n_frames == 0 clears a pending table.  The
 *                        table belongs to the NEXT uis_decode / uis_decode_f64 / uis_decode_device on this handle, in
 *                        that call's frame order (utterance-major), and must hold exactly that call's frame count (else
 *                        that call returns UIS_ERR_INVALID_ARG and nothing runs).  The call consumes it whether it
 *                        succeeds or not; a call without a pending table decodes without one, whatever an earlier call
 *                        used.
 *
 * Refused with UIS_ERR_UNSUPPORTED, the table consumed and the handle usable: every uis_stream_* call made while a table
 * is pending (a session's tags arrive through uis_stream_speakers, below), uis_score_labels and uis_score_speakers (their labels
 * are given), and a decode whose test_iteration * N reaches 2^24 (a cluster's tag shares its block-count word).  The
 * refused call has done nothing but drop the table -- and whatever other pending table it would have consumed
 * (uis_frame_bias, uis_decode_limits).  That holds for uis_stream_end as well: refused, it leaves the session OPEN, and
 * the same call made again (no table is pending any more) closes it; a caller whose cleanup path may run with a table
 * pending clears it first (uis_frame_speakers(h, NULL, 0)) or calls uis_stream_end twice.  A decode
 * with a table runs the kernels with the owner-side selects, as one with uis_frame_bias does: where the decode without
 * one reports k_decode_rs or k_decode_big<WS>, uis_last_decode_instantiation reports k_decode_resident or k_decode_big.
 */
int32_t uis_frame_speakers(uis_handle* h, const uint8_t* tags, int64_t n_frames);

/*
 * Minimum turn length: decode under "a speaker who takes the floor keeps it for at least m frames".
 *
 * min_turn[u] = m is utterance u's bound in decode steps; 0 and 1 mean no rule.  A hypothesis' RUN is the number of
 * most recent decode steps of its trace that carry its last label -- the whole trace, tiled test_iteration times, so a
 * run continues across the pass boundary.  At a step, a hypothesis that has a last label l and a run below m keeps the
 * loss of candidate l only: every other cluster and the new cluster get +inf, which every select drops.  A hypothesis
 * without a last label (the first step) has every candidate.  The last turn of an utterance may be shorter than m -- the
 * utterance simply ends -- and with test_iteration >= 2 the first turn of the RETURNED labels (the last N steps of the
 * trace) may look shorter, because its run began in the pass before.  Sub-step j of a look-ahead window uses the run of
 * the prefix it extends.  Nothing else changes -- the priors, the ddCRP terms, the float32 accumulation, the prune order,
 * the tie rules, max_speakers, uis_frame_bias, uis_frame_speakers -- and the rules hold together: a contradiction (two
 * different tags on an utterance's first two frames under m = 3) leaves an empty beam, reported as ever (labels -1, score +inf).
 * No table, or one of zeros and ones, gives today's decode bit for bit, device memory included.
 *
 *   uis_min_turn   min_turn: host int32 [n_utt], each in [0, 32767] (else UIS_ERR_INVALID_ARG and the pending table is
 *                  left as it was: the run shares the hypothesis' last-label word, 15 bits); NULL clears a pending
 *                  table.  The table belongs to the NEXT uis_decode / uis_decode_f64 / uis_decode_device on this
 *                  handle, which consumes it whether it succeeds or not and must have exactly n_utt utterances (else
 *                  that call returns UIS_ERR_INVALID_ARG and nothing runs).  A decode without a pending table has no
 *                  rule, whatever an earlier call used.
 *
 * Refused with UIS_ERR_UNSUPPORTED, the table consumed and the handle usable: uis_score_labels, uis_score_speakers and
 * every uis_stream_* call made while a table is pending (the table is a decode's; a session takes its rule per slot,
 * through uis_session_min_turn below).  The refused call has done nothing but drop the table and whatever other pending
 * table it would have consumed.  Where several pending tables are refused by one call, the one reported is
 * uis_frame_speakers', then this one, then uis_frame_bias', then uis_decode_limits', then uis_stream_speakers'.  A
 * decode in which some utterance has m >= 2 runs the kernels with the owner-side selects, as one with uis_frame_bias
 * does: where the decode without a table reports k_decode_rs or k_decode_big<WS>, uis_last_decode_instantiation
 * reports k_decode_resident or k_decode_big.
 */
int32_t uis_min_turn(uis_handle* h, const int32_t* min_turn, int32_t n_utt);

/*
 * Minimum turn length in streaming sessions.
 *
 * The rule is the one above, unchanged: a session whose slot u has the value m, pushed in any chunking and with silent
 * slots, is bit for bit the uis_decode of the same frames under uis_min_turn's m at look_ahead 1 and test_iteration 1 --
 * labels, scores, the final beam and the n-best rows.  The value is a property of the session's SLOTS, as max_speakers
 * is: uis_stream_restart keeps it, blobs do not carry it, an imported utterance decodes on under the target slot's.
 * A hypothesis' run rides in the last-label word the session already keeps (the label in bits 0 .. 15, the run,
 * saturating at m, in bits 16 .. 30), so it follows the utterance through uis_stream_commit, uis_stream_retire and
 * uis_stream_export / _import and ends at uis_stream_restart.  A slot whose value is 0 or 1 never holds run bits, and a
 * session in which no slot has m >= 2 is the session without the call, to the byte: device tables and blobs.
 *
 *   uis_session_min_turn      min_turn: host int32 [n_utt of the session], each in [0, 32767]; 0 and 1: no rule.  A
 *                             value may differ from the slot's current one only while the slot's utterance has received
 *                             no frame (after uis_stream_begin or uis_stream_restart: nothing pushed, primed or
 *                             imported); otherwise, and for a value out of range, UIS_ERR_INVALID_ARG and NO slot
 *                             changes.  A session call between launches: a UIS_FLAG_PERSISTENT session honours the rule
 *                             (its resident launch leaves, the next push starts one under the new table).
 *   uis_session_get_min_turn  out: host int32 [n_utt]: the table as given (all 0 after uis_stream_begin).
 *   uis_session_turns         out: host int32 [n_utt][2]: {the last label of utterance u's best hypothesis, in the
 *                             numbering of uis_stream_labels' labels at this moment; its run}.  The run is 0 where the
 *                             slot has no rule; {-1, 0} without a live hypothesis (an emptied beam, the cluster cap,
 *                             nothing received).  With m >= 2 the speaker may change at the next frame iff run >= m.
 *                             Changes nothing.
 *
 * All three need an open session and, like every session call, refuse a pending uis_min_turn table.
 *
 * uis_stream_prime into a slot with m >= 2 gives the primed hypothesis the run min(trailing run of the prefix labels, m);
 * turns shorter than m INSIDE the prefix are the caller's and are kept.  uis_stream_retire reads the label of the word:
 * the cluster a live hypothesis is speaking in is never retirable, whatever its run, and the clusters above a retired
 * one move down under unchanged run bits.  Blobs: format 1, unchanged; export is verbatim.  uis_stream_import checks the
 * LABEL of every rank's word against its cluster count (a rank without clusters holds -1 exactly) and normalises the
 * run against the target slot's m: m < 2 gives the bare label; a word without a run (a blob from a slot without a
 * rule: nothing is known of the turn, so the past sets no constraint) gets run m; else min(run, m).  So
 * export(import(b)) == b wherever source and target slots have the same value.
 */
int32_t uis_session_min_turn(uis_handle* h, const int32_t* min_turn);
int32_t uis_session_get_min_turn(uis_handle* h, int32_t* out);
int32_t uis_session_turns(uis_handle* h, int32_t* out /* [n_utt][2] */);

/*
 * Known speakers in streaming sessions.
 *
 * The rule is the one above, unchanged: a session pushed under tags, in any chunking and with silent slots, is bit for
 * bit the uis_decode of the same frames under the same tags at look_ahead 1 and test_iteration 1 -- labels, scores, the
 * final beam and the n-best rows.  A hypothesis' binding lives in the session's tables between the calls, so it follows
 * the utterance through uis_stream_commit, uis_stream_retire and uis_stream_export / _import, and ends with it at
 * uis_stream_restart (the slot's next utterance starts unbound).
 *
 *   uis_stream_speakers  tags: host uint8 [n_frames], each in 0 .. 127 (a larger value: UIS_ERR_INVALID_ARG, and the
 *                        pending table stays as it was); tags == NULL or n_frames == 0 clears a pending table.  The
 *                        table belongs to the NEXT uis_stream_push or uis_stream_prime on this handle, in that call's
 *                        own frame order (utterance by utterance, then the chunk's frames), and must hold exactly that
 *                        call's frame count (else that call returns UIS_ERR_INVALID_ARG and the session is untouched).
 *                        That call consumes the table whether it succeeds or not.  Every OTHER uis_stream_* call made
 *                        while the table is pending leaves it pending: it waits for the next push or prime (or for
 *                        uis_stream_speakers(h, NULL, 0)), across uis_stream_labels, _commit, _end and _begin alike.
 *                        An all-zero table gives the push without one bit for bit.  Tags, a uis_frame_bias table and
 *                        uis_stream_limits may all be in force in one push.
 *
 * uis_stream_prime with a table binds the primed hypothesis as the decode would along the given labels.  Within one
 * utterance's prefix the relation tag <-> label must be a partial bijection -- one tag never on two labels, one label never
 * under two tags -- else UIS_ERR_INVALID_ARG ("the prefix labels contradict its tags") and the session is as it was.
 *
 * A UIS_FLAG_PERSISTENT session takes no tags: a push or a prime with a table, and the import of a blob that carries
 * tags, return UIS_ERR_UNSUPPORTED; the table is dropped and the session stays usable.
 *
 * A session is TAGGED once a push, a prime or an import has given it a non-zero tag, until uis_stream_end.  A tagged
 * session refuses, with UIS_ERR_UNSUPPORTED and before any device work, a push, prime or import that would bring any
 * utterance's frames received (committed ones included) to 2^24 or more: a cluster's tag shares its block-count word.
 *
 * Retirement: a cluster that carries a tag in any live hypothesis can still be named by the next tagged frame, so it is
 * not retirable -- a query does not list it, a list that names it is refused as any other cluster in use.  The clusters
 * above a retired one move down with their tags.  A name therefore keeps its cluster for the life of the utterance, one
 * utterance holds at most 127 names, and max_clusters has to leave room for them: that is the caller's business.
 *
 * Blobs: the format is unchanged and a blob without tags is byte-identical to what it was; the tags travel in the
 * block-count words.  uis_stream_import refuses a blob in which one hypothesis binds a tag twice, or that carries a tag
 * with 2^24 frames received or more.
 *
 *   uis_stream_bindings  out: host int32 [n_utt][128].  out[u][g], g = 1 .. 127: the cluster the best hypothesis of
 *                        utterance u binds tag g to, in the numbering of uis_stream_labels' labels at this moment; -1:
 *                        unbound.  out[u][0]: the number of bound tags.  An utterance without a live hypothesis (an
 *                        emptied beam, the cluster cap) gives 0 and -1 everywhere.  Changes nothing.
 */
int32_t uis_stream_speakers(uis_handle* h, const uint8_t* tags, int64_t n_frames);
int32_t uis_stream_bindings(uis_handle* h, int32_t* out /* [n_utt][128] */);

/*
 * Primed sessions: start the online decode of an open session's utterances from a LABELED PREFIX (enrolment,
 * a corrected opening, a recording continued across a seam).  Afterwards the session is in the state it would
 * hold had it received the prefix frames and its beam contained only the given hypothesis: the state
 * _update_beam_state (uisrnn/uisrnn.py:388-453) leaves along that trace, formed with the decode's own
 * arithmetic.  Every later uis_stream_push / _labels / _nbest behaves as in any session: labels are the prefix
 * followed by what is decoded, scores the prefix's negative log-likelihood plus the continuation, and
 * uis_stream_nbest's stable_out is at least the prefix length.
 *   frames, offsets : host, packed as for uis_score_labels; offsets is [n_utt + 1] for the SESSION's n_utt.
 *                     Utterance u's prefix has P_u = offsets[u+1] - offsets[u] frames; P_u = 0 leaves that
 *                     utterance exactly as it is.  Prefix frames count against the session's max_frames
 *   labels     : host int32 [offsets[n_utt]], first-appearance form per utterance
 *   scores_out : host float32 [n_utt] or NULL: the prefix's negative log-likelihood (what uis_score_labels gives,
 *                bit for bit), 0 where P_u = 0
 * All or nothing -- after an error no utterance has changed and the session stays usable:
 *   UIS_ERR_INVALID_ARG  no session; offsets[0] != 0 or decreasing; an utterance with P_u > 0 that has already
 *                        received (or been primed with) frames; P_u > max_frames; a negative label or one past
 *                        first-appearance form (a prefix cannot be an invalid trace); a prefix whose negative
 *                        log-likelihood is not finite (the message names the utterance)
 *   UIS_ERR_CLUSTER_CAP  a prefix with more clusters than the session's max_clusters
 *   UIS_ERR_OOM          as uis_score_labels
 * In a UIS_FLAG_PERSISTENT session the resident launch leaves the device for this call (as for
 * uis_stream_nbest) and the next push starts a new one.  It leaves once the checks of the arguments have
 * passed and before the prefix is run (the launch occupies every compute unit): a call refused for a
 * non-finite likelihood or with UIS_ERR_OOM leaves every table as it was but has cost the resident launch;
 * one refused for its arguments (everything else above) has not.
 */
int32_t uis_stream_prime(uis_handle* h, const float* frames, const int64_t* offsets,
                         const int32_t* labels, float* scores_out);

/*
 * Sequence-match accuracy on the device -- the step after predict() in the reference's demo
 * (demo.py:61-66; uisrnn/evals.py:40-73: confusion matrix + scipy linear_sum_assignment).
 * For every utterance u (labels offsets[u] .. offsets[u+1] of both sequences) matched_out[u]
 * = the number of positions that agree under the best one-to-one mapping between the two
 * label sets; accuracy = matched_out[u] / length in float64 (evals.py:72), left to the caller.
 * Labels are int32 in [0, 65536) (map other id types to integers first, as evals.py:58-61
 * does), at most 64 distinct values per sequence -- otherwise UIS_ERR_UNSUPPORTED.  Empty
 * utterances give 0 (the reference raises ValueError there; the Python mirror does too).
 *   uis_eval_accuracy         both sequences on the host
 *   uis_eval_accuracy_device  both in HBM on the handle's device
 *   uis_eval_last_decode      sequence a = the labels of this handle's last successful
 *                             uis_decode, still resident in HBM; truth: host, same packing
 * offsets / matched_out are host pointers.
 */
int32_t uis_eval_accuracy(uis_handle* h, const int32_t* labels_a, const int32_t* labels_b,
                          const int64_t* offsets, int32_t n_utt, int64_t* matched_out);
int32_t uis_eval_accuracy_device(uis_handle* h, const int32_t* d_labels_a, const int32_t* d_labels_b,
                                 const int64_t* offsets, int32_t n_utt, int64_t* matched_out);
int32_t uis_eval_last_decode(uis_handle* h, const int32_t* truth, int32_t n_utt, int64_t* matched_out);

/*
 * The model's negative log-likelihood of a GIVEN labeling: the neg_likelihood the beam search
 * minimises (uisrnn/uisrnn.py:388-453) along the fixed trace labels[offsets[u] .. offsets[u+1]) of
 * every utterance, from an empty BeamState, test_iteration 1.  For labels that a decode with
 * test_iteration 1 returns (any beam_size / look_ahead), scores_out[u] equals that decode's score
 * bit for bit: both follow include/uis_numerics.h, the total is ((0 + loss_0) + loss_1) + ... in
 * float32, frame order.
 *   frames, offsets : host, packed as for uis_decode (float32, already cast)
 *   labels  : host, int32 [offsets[n_utt]], in first-appearance form (each label at most one more
 *             than the largest before it in its utterance).  A larger one makes that utterance +inf
 *             from that frame on (the reference's invalid trace, uisrnn.py:406-408); a negative one
 *             is UIS_ERR_INVALID_ARG
 *   scores_out       : host float32 [n_utt] or NULL; an empty utterance scores 0
 *   frame_losses_out : host float32 [offsets[n_utt]] or NULL -- each frame's step loss
 * Refused while a streaming session is open.  Leaves the last decode's results alone
 * (uis_last_decode_info / _shape, uis_eval_last_decode, uis_debug_scores).  UIS_ERR_OOM: score
 * the list in parts.
 */
int32_t uis_score_labels(uis_handle* h, const float* frames, const int64_t* offsets, int32_t n_utt,
                         const int32_t* labels, float* scores_out, float* frame_losses_out);

/*
 * Every speaker's per-frame loss along a GIVEN labeling: for frame t of an utterance, the row _update_beam_state
 * (uisrnn/uisrnn.py:388-453) would charge for assigning the frame to each open cluster, or to a new one, given the
 * labeled history before t -- the _calculate_score row along the fixed trace, of which uis_score_labels'
 * frame_losses_out is the chosen column.  With K(t) = the clusters opened by the frames before t:
 *   losses_out[t * width + k], k <  K(t) : step loss of (weighted MSE of x_t against cluster k's running mean as it
 *                                          stands before frame t, prior lp_stay if k is the previous frame's label,
 *                                          else (lp_sw + log blk_k) - log(sum blk + alpha))
 *                              k == K(t) : the new-speaker candidate (MSE against m0, lp_new - log(sum blk + alpha))
 *                              k >  K(t) : +inf (the padding of _calculate_score and uis_debug_scores)
 * and every row from the first label past the allowed range on is all +inf (the invalid trace).  Priors in float64 with
 * the decode's expressions and log tables, the MSE in the order of include/uis_numerics.h, so that
 *   1. losses_out[t * width + labels[t]] equals uis_score_labels' frame_losses_out[t] bit for bit, and
 *   2. for the labels of a beam_size 1, look_ahead 1, test_iteration 1 decode, float32(cum_{t-1} + row t) equals that
 *      decode's uis_debug_scores row of step t bit for bit (cum_t = float32(cum_{t-1} + losses_out[t][labels[t]])).
 *   frames, offsets, labels : as uis_score_labels
 *   width      : columns per row, at least (clusters of the utterance's valid trace) + 1 for every utterance and at
 *                least 1 -- otherwise UIS_ERR_INVALID_ARG, before any device work
 *   losses_out : host float32 [offsets[n_utt]][width]
 *   scores_out : host float32 [n_utt] or NULL: what uis_score_labels gives, bit for bit
 * Refusals and side effects as uis_score_labels: refused while a streaming session is open, leaves the last decode's
 * results alone, UIS_ERR_OOM: score the list in parts.
 */
int32_t uis_score_speakers(uis_handle* h, const float* frames, const int64_t* offsets, int32_t n_utt,
                           const int32_t* labels, int32_t width, float* losses_out, float* scores_out);

/*
 * Speaker profiles: who the speakers of a GIVEN labeling are.  Utterance u has K_u clusters;
 * cluster k holds frames t_1 < ... < t_n, counted from the utterance's first frame.
 *   frames, offsets, labels : as uis_score_labels
 *   width          : rows per utterance, at least every utterance's cluster count (of its valid trace) and at least 1
 *                    -- otherwise UIS_ERR_INVALID_ARG, before any device work, and the handle stays usable
 *   n_clusters_out : host int32 [n_utt]: K_u; -1 for an invalid trace (a label past the allowed range, the trace
 *                    uis_score_labels scores +inf)
 *   stats_out      : host int32 [n_utt][width][4]: {n, blocks, t_1, t_n}; blocks = the maximal runs of k in the labels
 *                    (the ddCRP block count)
 *   mean_out       : host float32 [n_utt][width][D]: the cluster's running mean of linear_mean2 outputs after its last
 *                    frame -- what every later frame of the speaker would be scored against, and the bits
 *                    uis_stream_prime leaves in the session's pool for that cluster
 *   sum_x_out      : host float32 [n_utt][width][D] or NULL: ((0 + x[t_1]) + x[t_2]) + ..., float32, frame order
 *   sum_r2_out     : host float32 [n_utt][width][D] or NULL: acc = +0; for j = 1 .. n: r = x[t_j] - P_j, acc = acc + r * r,
 *                    each operation rounded to float32; P_1 = the mean of a fresh cluster (what a new speaker's MSE is
 *                    measured against), P_j = the running mean after frame t_{j-1}: the mean uis_score_labels charged
 *                    frame t_j against.  Summed over clusters and divided by the frame count it is the closed-form
 *                    maximum-likelihood sigma2 under the model's own means
 *   scores_out     : host float32 [n_utt] or NULL: what uis_score_labels gives, bit for bit (+inf for an invalid trace)
 * Only the D real dimensions are written.  Rows k >= K_u, and every row of an invalid trace, hold stats {0, 0, -1, -1}
 * and +0.0 in every float.  Non-finite observations propagate as the arithmetic above propagates them.  A pending
 * uis_frame_bias table is taken and reaches scores_out only.  Refusals and side effects as uis_score_labels; on top,
 * UIS_ERR_UNSUPPORTED, before any device work, when the utterances of one call hold more than 65535 clusters in all
 * (one grid row per cluster chain): profile the list in parts.
 */
int32_t uis_speaker_profiles(uis_handle* h, const float* frames, const int64_t* offsets, int32_t n_utt,
                             const int32_t* labels, int32_t width, int32_t* n_clusters_out, int32_t* stats_out,
                             float* mean_out, float* sum_x_out, float* sum_r2_out, float* scores_out);

/*
 * Speaker profiles of an open session: the speakers of each utterance's best hypothesis right now.  A session call
 * between launches, as uis_stream_bindings and uis_session_turns (the resident launch of a UIS_FLAG_PERSISTENT session
 * leaves and the next push starts it again); no bit of the session changes.  (Named uis_session_*, as uis_session_turns:
 * every other uis_stream_* call's rule applies -- pending limit / bias / stream-speaker tables stay pending, a pending
 * uis_frame_speakers or uis_min_turn table is refused.)
 *   width          : rows per utterance, at least the session's max_clusters -- otherwise UIS_ERR_INVALID_ARG
 *   n_clusters_out : host int32 [n_utt]: the clusters K of the rank-0 hypothesis; 0 for a slot that has received
 *                    nothing; -1 for an utterance without a live hypothesis (cluster-cap overflow, an emptied beam)
 *   stats_out      : host int32 [n_utt][width][4]: {frames the cluster has absorbed, its block count, its known-speaker
 *                    tag (0: none), 0}; cluster indices are uis_stream_labels' numbering at this moment
 *   mean_out       : host float32 [n_utt][width][D]: the cluster's running mean, from the session's pool
 * Rows past K (every row where K = -1): stats {0, 0, -1, -1}, +0.0 in every float.
 */
int32_t uis_session_profiles(uis_handle* h, int32_t width, int32_t* n_clusters_out, int32_t* stats_out, float* mean_out);

/*
 * N-best readout: the labels of EVERY hypothesis of the final beam, not only of rank 0.  A decode
 * leaves the back-pointers of all beam_size ranks and the final beam's scores on the device; these
 * calls only read them (no decode kernel is involved).
 *   n_best     : hypotheses wanted per utterance, in [1, beam_size of that decode / session]
 *   labels_out : host int32.  Utterance u with N_u frames owns
 *                labels_out[n_best * off[u] .. n_best * off[u+1]), off = the last decode's offsets
 *                (a session: prefix sums of the frames received); hypothesis k is the row at
 *                + k * N_u, trace[-N_u:] in the form of uis_decode's labels_out.  Row 0 equals what
 *                the decode / uis_stream_labels returned; rows k >= counts_out[u] hold -1
 *   capacity   : int32 slots at labels_out (n_best * off[n_utt] needed)
 *   scores_out : host float32 [n_utt * n_best] or NULL: the final beam's scores, ascending, +inf padded
 *   counts_out : host int32 [n_utt] or NULL: min(n_best, live hypotheses); 0 for an empty utterance, an
 *                emptied beam and an utterance flagged in the overflow word
 * uis_last_decode_nbest: after a uis_decode / uis_decode_f64 / uis_decode_device that returned UIS_OK or
 * UIS_ERR_CLUSTER_CAP, whichever kernels decoded; any number of times, also after uis_score_labels and
 * uis_eval_*; it leaves uis_last_decode_info / _shape and uis_eval_last_decode alone.
 * UIS_ERR_INVALID_ARG: no such decode, a session is open, n_best or capacity out of range -- and after a
 * session that called uis_stream_labels: that call makes the session what uis_last_decode_info / _shape
 * describe, so the earlier decode's hypotheses are given up with it (the three always answer for one decode).
 * uis_stream_nbest: in an open session, for everything received so far.
 *   stable_out : host int64 [n_utt] or NULL: the number of leading frames on which all live hypotheses
 *                share one ancestor.  Every later beam descends from the current one, so
 *                uis_stream_labels' first stable_out[u] labels never change again (a guarantee, not a
 *                latency promise: a wide beam can keep an early alternative alive for long)
 * In a UIS_FLAG_PERSISTENT session the resident launch leaves the device for this call and the next
 * push starts a new one.  Returns UIS_ERR_CLUSTER_CAP (everything still written) if a cap was hit.
 */
int32_t uis_last_decode_nbest(uis_handle* h, int32_t n_best, int32_t* labels_out, int64_t capacity,
                              float* scores_out, int32_t* counts_out);
int32_t uis_stream_nbest(uis_handle* h, int32_t n_best, int32_t* labels_out, int64_t capacity,
                         float* scores_out, int32_t* counts_out, int64_t* stable_out);

/*
 * Posterior readout: how sure the decoder is of a label, or of a speaker turn, from the same records.  Per
 * utterance, over the `live` hypotheses uis_*_nbest(n_best = beam_size) would count, with their float32 scores
 * s_0 <= s_1 <= ... and labels lab_k[t] over the N frames of the readout (trace[-N:]; a session: the window):
 *   w_k           = exp(-(s_k - s_0) / temperature) / sum_j exp(-(s_j - s_0) / temperature)
 *   confidence[t] = sum_k w_k [lab_k[t] == lab_0[t]]    the beam's posterior mass behind the label returned.
 *                   Label agreement, not permutation invariant: an early extra cluster in an alternative
 *                   hypothesis lowers the agreement of all later frames
 *   change[t]     = sum_k w_k [lab_k[t] != lab_k[t-1]]  the posterior of a speaker turn between frames t-1 and
 *                   t; invariant to how a hypothesis numbers its speakers.  change[0] = 0 always: the first
 *                   frame of the readout has no predecessor IN the readout -- also the first frame of a committed
 *                   window and with test_iteration > 1
 *   temperature    : finite and > 0; 1 is the model's own posterior.  A peaked model needs a larger one to rank
 *                    its uncertain frames (at D = 256 every weight but w_0 is usually below 1e-11 at 1)
 *   confidence_out,
 *   change_out     : host float32, `capacity` floats each, packed in utterance order like uis_decode's labels_out
 *                    (a session: like uis_stream_labels); either may be NULL
 *   weights_out    : host float32 [n_utt * beam_size] or NULL: w_k in rank order, 0 past live
 *   counts_out     : host int32 [n_utt] or NULL: live
 * live == 0 (an empty utterance, an emptied beam, an utterance flagged in the overflow word): zeros and count 0.
 * live == 1: confidence is exactly 1.0f, change exactly 0.0f or 1.0f.  A session window that a commit emptied:
 * count 1, weights_out[u * beam_size] = 1, no frames.  Two calls on the same state return the same bits.
 * Validity, refusals and status are those of the n-best pair (uis_last_decode_posterior: a decode that returned
 * UIS_OK or UIS_ERR_CLUSTER_CAP and no open session; uis_stream_posterior: an open session, UIS_ERR_CLUSTER_CAP
 * with everything still written, the resident launch of a UIS_FLAG_PERSISTENT session leaves for the call).
 * UIS_ERR_INVALID_ARG (nothing touched): also a temperature that is not finite and > 0, capacity below the
 * frames in the readout.  The calls leave uis_last_decode_info / _shape, uis_eval_last_decode and a following
 * uis_*_nbest alone.
 */
int32_t uis_last_decode_posterior(uis_handle* h, double temperature, float* confidence_out, float* change_out,
                                  int64_t capacity, float* weights_out, int32_t* counts_out);
int32_t uis_stream_posterior(uis_handle* h, double temperature, float* confidence_out, float* change_out,
                             int64_t capacity, float* weights_out, int32_t* counts_out);

/*
 * Session commits: endless online decoding in a fixed window.  uis_stream_commit hands out the labels of an open
 * session that are final, drops their back-pointer records and gives the room back: max_frames is then the WINDOW,
 * the frames received and not yet committed, and a stream of any length can be pushed through it.  From the first
 * commit on, uis_stream_push's capacity check, uis_stream_labels, uis_stream_nbest and its stable_out all speak
 * about the window (committed labels are the caller's to keep: window labels follow them).  A session that never
 * commits behaves exactly as before.  No decode kernel is involved.  Per utterance u, with have = the frames in the
 * window and stable = what uis_stream_nbest reports:
 *   cut     horizon == NULL or horizon[u] < 0: cut = stable.  Otherwise cut = max(stable, have - horizon[u]): frames
 *           older than the newest horizon[u] are decided in favour of the best hypothesis (a decision horizon, the
 *           bound on the delay that the stable prefix alone does not give)
 *   prune   only if cut > stable: every live hypothesis whose ancestor at step cut - 1 is not rank 0's -- whose
 *           labels differ from rank 0's somewhere in [0, cut) -- leaves the beam.  Survivors keep their order, their
 *           scores and all their state; rank 0 always survives; horizon[u] == 0 collapses the beam onto rank 0.
 *           dropped_out[u] = the number removed
 *   commit  c = cut & ~1 (even, so the beam tables keep the parity of the step count).  labels_out receives rank 0's
 *           labels of window frames [0, c), packed in utterance order; counts_out[u] = c.  The window then starts c
 *           frames later.  Cluster ids stay what they were: first-appearance form over the WHOLE stream
 * An utterance with nothing in its window, with an emptied beam or flagged in the overflow word commits 0 and is
 * left alone.  Scores are not rebased: they go on growing with the stream (float32).  A window that a commit has
 * emptied (c = have) holds exactly one hypothesis: until the utterance's next frame uis_stream_labels reports its
 * score with no labels, and uis_stream_nbest counts_out 1, that score, a row of no labels and stable_out 0.
 *   horizon     : host int32 [n_utt] or NULL
 *   labels_out  : host int32, capacity slots; capacity >= the frames in the window (sum over utterances)
 *   counts_out  : host int32 [n_utt]
 *   dropped_out : host int32 [n_utt] or NULL
 * All or nothing: UIS_ERR_INVALID_ARG (no session open, capacity too small) touches nothing; UIS_ERR_OOM (the prior
 * tables, which grow with the frames ever received, could not be lengthened) leaves the session as it was.  In a
 * UIS_FLAG_PERSISTENT session the resident launch leaves the device for this call (as for uis_stream_nbest) and the
 * next push starts a new one.  An utterance that has committed frames cannot be primed, also when its window is
 * empty; one cannot receive more than 2^31 - 256 frames in one session (uis_stream_push: UIS_ERR_UNSUPPORTED).
 * uis_stream_committed: committed_out host int64 [n_utt], the frames committed so far per utterance.
 */
int32_t uis_stream_commit(uis_handle* h, const int32_t* horizon, int32_t* labels_out, int64_t capacity,
                          int32_t* counts_out, int32_t* dropped_out);
int32_t uis_stream_committed(uis_handle* h, int64_t* committed_out);

/*
 * Session restarts: end some utterances of an open session and reuse their slots in place.  The set of utterances
 * of a session is fixed by uis_stream_begin; uis_stream_restart lets one of them end -- its final window labels are
 * handed out -- and leaves its slot in the state uis_stream_begin gives an utterance, so that the next stream can
 * use it while every other utterance's beam lives on untouched.  It is also how a dead slot comes back: one that
 * hit the cluster cap (its overflow word is set) or whose beam a non-finite frame emptied.  No decode kernel is
 * involved.
 *   which        : host int32 [n_utt]; non-zero = this utterance ends here
 *   labels_out   : host int32, capacity slots: exactly what uis_stream_labels would write at this moment for the
 *                  selected utterances -- rank 0's labels of the frames in their windows, packed in utterance order
 *                  (labels already committed are the caller's, as after any commit).  capacity >= the sum of window
 *                  frames over the selected utterances
 *   counts_out   : host int32 [n_utt]: window frames handed out, 0 for an utterance not selected
 *   scores_out   : host float [n_utt] or NULL: for selected utterances what uis_stream_labels reports (the kept
 *                  score of a window emptied by a commit, +inf for an emptied beam, 0 for nothing received);
 *                  entries of utterances not selected are not written
 *   overflow_out : host int32 [n_utt] or NULL: the selected utterances' overflow words BEFORE the reset; entries
 *                  not selected are not written
 * Afterwards every selected utterance has received nothing and committed nothing (uis_stream_committed reports 0),
 * holds one empty hypothesis of score 0, its overflow word is clear, uis_stream_prime accepts it, and its count
 * towards the 2^31 - 256 frame limit starts again.  Utterances not selected are untouched, to the bit.
 * Returns UIS_OK, or UIS_ERR_CLUSTER_CAP when a selected utterance had hit the cap: as in uis_stream_labels
 * everything is still written, and the restart has still happened.  Otherwise all or nothing: UIS_ERR_INVALID_ARG
 * (no session open, null which / counts_out, capacity too small, null labels_out with labels due) touches nothing;
 * UIS_ERR_OOM (scratch) leaves the session as it was.  Selecting nothing is UIS_OK with zero counts and no device
 * work.  The call does not change what uis_last_decode_info / _shape answer for; like a commit it invalidates the
 * n-best cache.  In a UIS_FLAG_PERSISTENT session the resident launch leaves the device for this call (after the
 * host checks, as for uis_stream_commit) and the next push starts a new one.  UIS_POISON_WORKSPACE: everything the
 * ended stream leaves behind in the slot (its back-pointer rows, pool slots and beam-table rows) is filled with the
 * word before the reset.  UIS_RESTART_TRACE=1: one line per call on stderr.
 */
int32_t uis_stream_restart(uis_handle* h, const int32_t* which, int32_t* labels_out, int64_t capacity,
                           int32_t* counts_out, float* scores_out, int32_t* overflow_out);

/*
 * Speaker retirement: keep an endless session under max_clusters.  uis_stream_commit gives back the room of old
 * frames; the cluster tables of a hypothesis only grow, and a step that selects a new cluster at K == max_clusters
 * sets the utterance's overflow word, after which only uis_stream_restart brings the slot back.  uis_stream_retire
 * deletes clusters that no live hypothesis can still name.  No decode kernel is involved (an addition: the ABI
 * version stays).  Per utterance, with have = the frames in the window: cluster index k is RETIRABLE iff for every
 * live hypothesis r  k < K_r,  k is not among r's labels of the window's frames,  and k is not r's last label (which
 * matters for a window that a commit emptied: its one hypothesis still continues from it).  Such a cluster was opened
 * before the window; after a commit or a prime all live hypotheses share that history, so k is the same speaker in
 * each.  A session that never committed and was not primed has nothing retirable.  Retiring a set R removes the
 * entries in R from every live hypothesis' cluster lists (the entries above move down in order), K -= |R|, the sum of
 * block counts loses those of R, the last label and every label of the window's records become
 * label - #{k in R : k < label}; scores, the step count and the prior tables stay.  The decode continues exactly as
 * the reference's beam search would from hypotheses with those clusters deleted: the ddCRP denominator
 * sum(block counts) + alpha shrinks accordingly, so FOR THE PRIOR THE SPEAKER NEVER EXISTED (the one modelling
 * decision of this call).  Cluster ids of labels handed out afterwards are in the NEW numbering: the caller keeps the
 * map (uisrnn_amd.OnlineSession does: ids it hands out never change and are never reused).
 *   which, offsets, clusters : the selection.
 *                  offsets == NULL (then clusters == NULL): every retirable cluster of every utterance with
 *                  which[u] != 0 (which == NULL: of every utterance); the others are only queried.
 *                  offsets != NULL (then which == NULL): host int64 [n_utt + 1], offsets[0] = 0, non-decreasing;
 *                  clusters host int32 [offsets[n_utt]], utterance u's indices at [offsets[u], offsets[u + 1]),
 *                  ascending.  An empty selection is a pure query
 *   retired_out  : host int32 [n_utt * max_clusters]: row u holds counts_out[u] indices, ascending, in the numbering
 *                  BEFORE the call.  May be NULL only when the selection is explicit and empty
 *   counts_out   : host int32 [n_utt]: clusters retired
 *   k_out        : host int32 [n_utt]: the largest K over the live hypotheses AFTER the call (how close the
 *                  utterance is to max_clusters); 0 without a live hypothesis
 *   retirable_out, retirable_counts_out : host int32 [n_utt * max_clusters] / [n_utt] or NULL: the retirable
 *                  indices BEFORE the call, rows as retired_out
 * An utterance that has received nothing, whose beam is empty or which is flagged in the overflow word has nothing
 * retirable, is left alone and reports 0: retirement does not revive a dead slot, it is how a live one avoids dying.
 * All or nothing: UIS_ERR_INVALID_ARG -- no session open, a list that is not ascending, repeats an index or leaves
 * [0, max_clusters), or, for ANY utterance, names an index that is not retirable -- leaves the whole session as it
 * was, to the bit; UIS_ERR_OOM (scratch) likewise.  Utterances with nothing retired are untouched, to the bit.  In a
 * UIS_FLAG_PERSISTENT session the resident launch leaves the device for this call (after the host checks, as for
 * uis_stream_commit) and the next push starts a new one.  UIS_RETIRE_TRACE=1: one line per call on stderr.
 */
int32_t uis_stream_retire(uis_handle* h, const int32_t* which, const int64_t* offsets, const int32_t* clusters,
                          int32_t* retired_out, int32_t* counts_out, int32_t* k_out, int32_t* retirable_out,
                          int32_t* retirable_counts_out);

/*
 * Export / import: one utterance of a live session as a blob of bytes, and back into a slot that has received
 * nothing -- another slot, another session (other n_utt, max_frames, max_clusters, flags), another handle, device or
 * process: checkpoints, moves out of a full session, rebalancing between ranks.  Between two pushes an utterance IS
 * its tables; the blob holds them and the three host words (window frames, committed, the score at the last commit),
 * every live hypothesis included, and the decode continues from an imported utterance bit for bit as it would have
 * in the source.  No decode kernel is involved (an addition: the ABI version stays).  One utterance per call.
 *   uis_stream_export_bound : host only, no device work.  bytes_out: the capacity uis_stream_export asks for (the
 *                  largest blob a session of this shape can give).
 *   uis_stream_export : blob host memory of `capacity` >= that bound bytes; bytes_out: the bytes written (usually far
 *                  fewer).  Read-only: no table and no host word of the session changes.  The blob is self-describing
 *                  (magic, format and numerics versions, a model fingerprint: the shape and a 64-bit hash of the
 *                  parameters as uis_create received them, beam_size), position-independent, ends in a checksum, and
 *                  CANONICAL: it depends on the utterance's state alone, not on the slot or session it sat in, so
 *                  export(import(blob)) == blob byte for byte.  csrc/uis_blob.h states the layout.  An utterance that
 *                  has received nothing exports a valid blob (the empty hypothesis).  Refused, nothing written:
 *                  UIS_ERR_CLUSTER_CAP for an utterance flagged in the overflow word, UIS_ERR_INVALID_ARG for one
 *                  whose beam a non-finite frame emptied (there is nothing to move: uis_stream_restart is the way
 *                  back), for utt out of range and for a capacity below the bound.
 *   uis_stream_import : all or nothing.  The target utterance must have received nothing (uis_stream_prime's rule).
 *                  Must match: the model fingerprint, UIS_NUMERICS_VERSION, beam_size.  Must fit: the window's frames
 *                  <= max_frames, every hypothesis' clusters <= max_clusters (UIS_ERR_CLUSTER_CAP otherwise; equality
 *                  is accepted, as in uis_stream_prime), its pool slots <= those of the target.  Everything else is
 *                  UIS_ERR_INVALID_ARG: a blob that is cut short, damaged (checksum) or inconsistent in anything that
 *                  steers an address or a loop bound -- all decided on the host, before the device is touched; a call
 *                  refused so costs a UIS_FLAG_PERSISTENT session nothing.  Record words are taken as they are (their
 *                  readers clamp).  The session's prior tables grow where the utterance's history needs it, as in
 *                  uis_stream_commit, and the 2^31 - 256 frame limit goes on counting from the imported total.
 * In a UIS_FLAG_PERSISTENT session the resident launch leaves the device for both calls (after the host checks) and
 * the next push starts a new one.  UIS_MIGRATE_TRACE=1: one line per call on stderr.
 */
int32_t uis_stream_export_bound(uis_handle* h, int32_t utt, int64_t* bytes_out);
int32_t uis_stream_export(uis_handle* h, int32_t utt, void* blob, int64_t capacity, int64_t* bytes_out);
int32_t uis_stream_import(uis_handle* h, int32_t utt, const void* blob, int64_t bytes);

/*
 * Pinned (page-locked) host memory for the frames / labels handed to uis_decode: with it the
 * H2D copy of the frame stream is asynchronous and overlaps the input projection of the chunks
 * already on the device.  Pageable memory works too (staged by the runtime).
 */
int32_t uis_host_alloc(size_t bytes, void** out);
void uis_host_free(void* p);

const char* uis_last_error(void);

/*
 * Training (reference: UISRNN.fit_concatenated's loop, uisrnn/uisrnn.py:254-296, and
 * uisrnn/loss_func.py).  A trainer handle is separate from uis_handle: it owns the weights
 * being trained, their gradients, the Adam state and the training sequences on one device.
 * The host (uisrnn_amd/training.py) prepares the data and draws each iteration's batch.
 *
 * Flat parameter order (uis_train_get_params / uis_train_get_grads), float32, row-major:
 *   for each layer l: gru_weight_ih[l] (3H, D|H), gru_weight_hh[l] (3H, H),
 *                     gru_bias_ih[l] (3H), gru_bias_hh[l] (3H)
 *   linear_mean1_weight (H, H), linear_mean1_bias (H),
 *   linear_mean2_weight (D, H), linear_mean2_bias (D),
 *   rnn_init_hidden (depth, H), sigma2 (D)
 * i.e. CoreRNN.parameters() order, then rnn_init_hidden, then sigma2.
 */
typedef struct uis_train_opts {
  double learning_rate;          /* Adam lr (beta 0.9 / 0.999, eps 1e-8, as torch.optim.Adam)   */
  double regularization_weight;  /* loss3 = weight * sum of the Frobenius norms of CoreRNN's params */
  double grad_max_norm;          /* clip_grad_norm_ over CoreRNN's params                         */
  double sigma_alpha;            /* inverse-gamma prior of sigma2                                 */
  double sigma_beta;
  double dropout;                /* between GRU layers (depth >= 2); 0 = none                     */
  uint64_t dropout_key;          /* key of the counter-based dropout stream                       */
  int32_t estimate_sigma2;       /* 1: Adam also updates sigma2                                   */
  int32_t reserved[3];
} uis_train_opts;

typedef struct uis_trainer uis_trainer;

/* A trainer on HIP device `device`, starting from the weights in `desc` with a fresh Adam state.
 * desc->transition_bias and crp_alpha are not used. */
int32_t uis_train_create(const uis_model_desc* desc, const uis_train_opts* opts, int32_t device,
                         uis_trainer** out);

/* Upload the training sub-sequences once.  pool: host, float32, [seq_offsets[n_seqs], D];
 * sub-sequence s owns rows seq_offsets[s] .. seq_offsets[s+1] (at least one row each). */
int32_t uis_train_set_data(uis_trainer* th, const float* pool, const int64_t* seq_offsets,
                           int32_t n_seqs);

/* One iteration on the batch of sub-sequences batch_idx[0 .. batch_size): their row counts must
 * be non-increasing.  The padded input is gathered on the device (row 0 zeros, then the rows).
 * out_losses (host, may be NULL): loss, loss1, loss2, loss3 -- with it the call waits for the
 * device; without it the iteration is only queued. */
int32_t uis_train_step(uis_trainer* th, const int32_t* batch_idx, int32_t batch_size,
                       float* out_losses);

/* Number of floats of the flat parameter vector (layout above). */
int32_t uis_train_param_count(uis_trainer* th, int64_t* count_out);

/* Current weights / the gradients of the last iteration (after clipping), flat layout above. */
int32_t uis_train_get_params(uis_trainer* th, float* params_out, int64_t count);
int32_t uis_train_get_grads(uis_trainer* th, float* grads_out, int64_t count);

void uis_train_destroy(uis_trainer* th);

#ifdef __cplusplus
}
#endif
#endif /* UISRNN_HIP_H_ */
