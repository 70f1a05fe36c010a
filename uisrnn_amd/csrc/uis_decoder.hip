// uis_decoder.hip -- host side of libuisrnn_hip.so: the C ABI of include/uisrnn_hip.h.
//
// Replaces, for the decode path only, what the reference does in
//   UISRNN.__init__/load  (weights in)            uisrnn/uisrnn.py:83-107,149-170
//   UISRNN.predict / predict_single (beam search) uisrnn/uisrnn.py:479-590
// Utterances advance in lock-step: per step one select launch (one workgroup
// per utterance) and one batched CoreRNN evaluation over the surviving
// hypotheses of ALL utterances (GRU GEMM, mean-head GEMMs).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>
// (host pass only, x86 only: the float64 -> float32 cast below writes around the cache with SSE2 streaming
// stores; any other host takes the scalar loop, same rounding)
#if !defined(__HIP_DEVICE_COMPILE__) && (defined(__SSE2__) || defined(__x86_64__))
#define UIS_HOST_SSE2 1
#include <emmintrin.h>
#endif

#include "uis_poison.h"
#include "uis_blob.h"
#include "uis_call_tables.h"
#include "uis_push_layout.h"
#include "uis_kernels.hip"
#include "uis_eval.hip"
#include "uisrnn_hip.h"

#define UIS_EXPORT extern "C" __attribute__((visibility("default")))

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIPCHK(expr)                                                                   \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess)                                                              \
      return fail(e_ == hipErrorOutOfMemory ? UIS_ERR_OOM : UIS_ERR_HIP,               \
                  std::string(#expr) + ": " + hipGetErrorString(e_));                  \
  } while (0)

// (what uis_call_tables.h reports, as this file's calls return it)
int table_status(const TableStatus& s) { return s.code == UIS_OK ? UIS_OK : fail(s.code, s.msg); }

int round_up(int v, int m) { return (v + m - 1) / m * m; }

// Device memory that frees itself (move-only).  ensure() grows it and never shrinks it; alloc() is one allocation of
// exactly `bytes`; view() makes it a window into someone else's allocation (`borrowed`: never freed from here).
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  bool borrowed = false;  // a view into the handle's workspace arena, not an allocation of its own
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept { swap(o); }
  DevBuf& operator=(DevBuf&& o) noexcept { swap(o); return *this; }  // (o's destructor frees what this one held)
  ~DevBuf() { release(); }
  void swap(DevBuf& o) { std::swap(p, o.p); std::swap(cap, o.cap); std::swap(borrowed, o.borrowed); }
  int alloc(size_t bytes) {
    release();
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
      p = nullptr;
      return fail(UIS_ERR_OOM, "hipMalloc of " + std::to_string(bytes) + " bytes failed: " + hipGetErrorString(e));
    }
    cap = bytes;
    return UIS_OK;
  }
  int ensure(size_t bytes) {
    if (borrowed) release();
    return bytes <= cap ? UIS_OK : alloc(bytes + bytes / 8 + 256);
  }
  void view(void* at, size_t bytes) { release(); p = at; cap = bytes; borrowed = true; }
  void release() { if (p && !borrowed) (void)hipFree(p); p = nullptr; cap = 0; borrowed = false; }
  template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

// The same for pinned host memory.  ensure() allocates exactly `bytes` when the block is smaller (the caller adds its
// own head-room where a block grows often) and leaves the HIP error to the caller: some can do without the block.
struct HostBuf {
  void* p = nullptr;
  size_t cap = 0;
  HostBuf() = default;
  HostBuf(HostBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); }
  HostBuf& operator=(HostBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
  ~HostBuf() { release(); }
  hipError_t ensure(size_t bytes, unsigned flags) {
    if (bytes <= cap) return hipSuccess;
    release();
    hipError_t e = hipHostMalloc(&p, bytes, flags);
    if (e != hipSuccess) { p = nullptr; return e; }
    cap = bytes;
    return hipSuccess;
  }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
  template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

// Device allocations of a one-off call (uis_rnn_step, the bootstrap of uis_create): freed on every
// return path.
struct Scratch {
  std::vector<void*> ptrs;
  ~Scratch() { for (void* p : ptrs) (void)hipFree(p); }
  template <typename T> int get(T** out, size_t count) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T));
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? UIS_ERR_OOM : UIS_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    ptrs.push_back(p);
    *out = static_cast<T*>(p);
    return UIS_OK;
  }
};

#define UIS_WIDE_TILE_ROWS 2048   // row capacity (about twice the rows actually run, after dedup) above which the 2x2 tiles win
#define UIS_WT_ROWS 1280          // row capacity above which the LDS-weight kernels (k_wt_*) take over at hidden size 256 / 512
#define UIS_MAX_GROUPS 8
#define UIS_MAX_CLUSTERS 16         // clusters of 32 CUs the one-launch decode can address
#define UIS_LEVEL_CAP 32768        // hypotheses per intermediate look-ahead level and utterance: the DEFAULT (uis_decode_opts.level_cap)
#define UIS_LEVEL_CAP_MAX 524287    // ... and the most a caller may ask for (window_body packs a level's hypothesis index into 19 bits)
#define UIS_WINDOW_WIDE_LEVEL 256  // level capacity (hypotheses) from which k_window runs with more threads per utterance
#define UIS_WINDOW_WIDE_NT 512   // (1024 measured the same)
#define UIS_GRAPH_STEPS 32   // decode steps per captured graph (even)
#define UIS_STREAM_RESIDENT_MIN_STEPS 4  // uis_stream_push: steps per push from which the one-launch kernel is used
#ifndef UIS_H2D_CHUNKS
#define UIS_H2D_CHUNKS 2     // uis_decode: host frames are copied in this many pieces, overlapped with the input projection (1 / 2 / 3 / 4 pieces measured: 1.505 / 1.517 / 1.424 / 1.43 M frames/s from pinned buffers at configs[1])
#endif
#ifndef UIS_F64_PIECES
#define UIS_F64_PIECES 4     // uis_decode_f64: copies per projection chunk (the cast runs ahead of them)
#endif
#ifndef UIS_H2D_MIN_FRAMES
#define UIS_H2D_MIN_FRAMES 4096  // ... of at least this many frames each
#endif

struct GraphCache {
  hipGraphExec_t exec = nullptr;
  DecodeState st{};
  size_t lds = 0;
};

struct ProfileEvents {
  std::vector<hipEvent_t> ev;   // pairs
  std::vector<int> cls;
  size_t used = 0;
};

// The chunk of a streaming push: the frames it brings and what is formed of them once per chunk, a row per frame.  Grow only; a UIS_FLAG_PERSISTENT session takes it at full size when it opens.
struct Chunk {
  // one push = one H2D copy: the block ChunkLayout describes ([k_ingest's table, tensors only][foff][avail][frames]) is
  // built in `stage` (pinned; for tensors without the frames, which the gather writes) and mirrored at the front of `x`
  HostBuf stage;
  // pad [rows][Dp] float32: the frames padded, where D != Dp; gi0 [rows][G], mse0 [rows] float32: the chunk's input
  // projection; bias [rows][3] float64: DecodeState::bias3 of a push with a uis_frame_bias table; hint [rows] uint8:
  // DecodeState::hint of a push with a uis_stream_speakers table
  DevBuf x, pad, gi0, mse0, bias, hint;
  // what a push of this layout needs; bias / hint where it has that table, the staging block (with head-room: pushes of
  // a session vary in size) unless the frames travel through the mailbox
  int ensure(const ChunkLayout& lay, size_t F, const DevModel& m, bool with_bias, bool with_hint, bool staged = true) {
    const size_t travel = staged && lay.travel_bytes > stage.cap ? lay.travel_bytes + lay.travel_bytes / 4 + 4096 : 0;
    if (hipError_t e = stage.ensure(travel, hipHostMallocDefault)) return fail(UIS_ERR_OOM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    int rc;
    if ((rc = x.ensure(lay.total_bytes)) || (rc = gi0.ensure(F * m.G * 4)) || (rc = mse0.ensure(F * 4)) ||
        (with_bias && (rc = bias.ensure(F * 24))) || (with_hint && (rc = hint.ensure(F)))) return rc;
    return m.D != m.Dp ? pad.ensure(F * m.Dp * 4) : UIS_OK;
  }
  // UIS_POISON_WORKSPACE: all of it, ahead of the defining writes
  hipError_t poison(const UisPoison& p, hipStream_t stream) {
    p.host(stage.p, stage.cap);
    for (DevBuf* b : {&x, &gi0, &mse0, &bias, &hint, &pad})
      if (hipError_t e = p.device(b->p, b->cap, stream)) return e;
    return hipSuccess;
  }
};

// What a streaming session owns: one move-assignment of a fresh one frees it all.
struct StreamMem {
  std::vector<DevBuf> allocs;  // the session's state, one allocation per table (uis_stream_begin)
  Chunk chunk;
  DevBuf labels, scores;  // uis_stream_labels' back-trace
  HostBuf pm_block;  // the persistent launch's mailbox (host-coherent; MailboxLayout)
  HostBuf h_land;    // the pinned landing block of every scaffold call's one download (session_buffers)
};

// Every device and pinned buffer of a handle outside its session, likewise.
struct HandleMem {
  // workspace (grow only)
  DevBuf off, utt_step, overflow, xpad, gi0, mse0, logblk, logden, pool_mean, pool_hid, pool_cnt;
  DevBuf beam_n, beam_K, beam_last, beam_sum, beam_score, beam_slot, beam_blk, bp, rows, nrows;
  DevBuf gi_up, a1, counters, beam_scores_out, io_frames, io_labels, io_scores, mse_tab, dbg_scores, utt_nrows, hst;
  DevBuf lv_n, lv_K, lv_last, lv_sum, lv_score, lv_origin, lv_path, lv_slot, lv_blk, scratch, bp16, bp_base, cluster_ctl, resume, split_tab, scatter_tab, stage;
  DevBuf limit, limit_in;  // [U] int32 each: DecodeState::limit, written by every decode, and uis_decode_limits' table it is written from
  DevBuf bias3;  // [frames][3] float64: DecodeState::bias3 of a decode with a uis_frame_bias table (the workspace's last view)
  DevBuf hint;   // [frames] uint8: DecodeState::hint of a decode with a uis_frame_speakers table (behind bias3: the workspace's last view)
  DevBuf min_turn;  // [U] int32: DecodeState::min_turn of a decode whose uis_min_turn table holds a value of 2 or more (behind hint: the workspace's last view)
  DevBuf rs_block;  // UIS_NO_ARENA: the stretch k_decode_rs addresses through one descriptor (pool_mean .. mse_tab), one allocation
  DevBuf arena;  // one allocation behind all of the above: the per-step tables share pages (TLB reach)
  HostBuf h_cast;  // uis_decode_f64: the pinned float32 staging buffer the utterances are cast into, chunk by chunk, ahead of each H2D copy
  HostBuf h_out;   // pinned landing block of uis_decode_f64's labels and scores
  DevBuf ev_a, ev_b, ev_off, ev_out;  // uis_eval_* staging
  DevBuf sc_x, sc_xpad, sc_gi0, sc_mse0, sc_loss, sc_prior, sc_hid, sc_a1, sc_mean, sc_gi_up, sc_rows, sc_chains, sc_utt, sc_out;  // uis_score_labels (its own: the last decode's buffers stay as they are)
  // uis_score_speakers' own: labels + each frame's row, logblk + logden, the candidate table [F][width] {mean row, block
  // count}, the frame table [F] {K, sum, last}, the rows [F][width]
  DevBuf sc_spk_in, sc_spk_log, sc_spk_cand, sc_spk_frame, sc_spk_loss;
  DevBuf sc_spk_bias;  // ... and the call's {lp_stay, lp_sw, lp_new} per frame, where uis_frame_bias left a table
  // uis_speaker_profiles' own: each chain's {output row, block count, first frame of its utterance}, the stats
  // [n_utt][width] {n, blocks, t_1, t_n}, and mean / sum_x / sum_r2, each [n_utt][width][D]
  DevBuf sc_prof_chain, sc_prof_stats, sc_prof_mean, sc_prof_sumx, sc_prof_sumr2;
  // the scratch block of one uis_stream_prime / _commit / _restart / _retire call (session_buffers in uis_stream.hip;
  // every such call synchronises before it returns, so no two are ever live; prime's forced run uses the sc_* above)
  DevBuf sc_session;
  DevBuf nb_labels, nb_scores, nb_counts, nb_stable, nb_off;  // the n-best readout's own
  // the posterior readout's own (a following n-best readout finds its buffers as it left them): results, offset tables,
  // the per-group partial rows of k_posterior; the label table and scores k_nbest_window fills for k_posterior_window
  DevBuf ps_conf, ps_change, ps_weights, ps_counts, ps_off, ps_part, ps_labels, ps_scores;
  // k_ingest's descriptor table (uis_ingest.hip): the pinned block it is built in and its device copy, one H2D per call
  DevBuf ingest_tab;
  HostBuf h_ingest;
};

// Which kernel-table entry a lookup returned (find_kernel fills it from the entry it found): the record behind
// uis_last_decode_instantiation.  k_decode_small and the launch-per-step path have no table: their family, variant 0.
struct KernelPick {
  int32_t family = 0 /* UIS_DK_* */, Hp = 0, Dp = 0, variant = 0, persist = 0 /* 1: from the persist table */;
};

}  // namespace

struct uis_handle : HandleMem {
  int device = 0;
  hipStream_t stream = nullptr, copy_stream = nullptr;
  std::vector<hipEvent_t> h2d_done;
  DevModel m{};
  std::vector<void*> model_allocs;
  double alpha = 1.0;
  uint64_t model_hash = 0;  // of the parameters as uis_create received them: the model fingerprint of uis_stream_export's blobs (uis_blob.h)
  int n_cu = 0;  // compute units of the device
  int hid_map_seg = 0, hid_map_seg_p = 0, H_model = 0;  // (round 6) HidMap of this model's hidden axis; rnn_hidden_size as the caller gave it
  // the one-launch decode relies on observed, not promised, placement (workgroup b on XCD b % 8,
  // all 256 workgroups resident); when its own checks fail once, this handle stops using it
  bool inlaunch_failed = false, resident_off = false;
  // Where the one-launch decode's control words (barrier and row counters of the clusters) sit
  // inside their buffer.  The kernel runs ~5 % faster or slower depending on address bit 13 / 20 of
  // that one 4 KB block (L2 channel hashing; which value is the good one depends on the physical
  // pages: tools/experiments/README.md), so the first decodes of a shape try the four placements
  // and the handle keeps the fastest.
  struct CtlTune {
    uint64_t sig = 0;     // shape the measurements belong to
    int phase = 0;        // 0: first (cold) decode of the shape; 1..4: trying placement phase-1; 5: decided
    int best = 0;
    float ms[4] = {0, 0, 0, 0};
  } ctl_tune;
  // streaming session (uis_stream_*): owns its device memory
  struct Stream : StreamMem {
    bool active = false;
    int U = 0, B = 0, Kmax = 0, S = 0;
    int64_t cap = 0;                  // frames per utterance the session can hold
    std::vector<int32_t> have;        // frames per utterance in the window: received or primed, not yet committed
    std::vector<int64_t> committed;   // frames per utterance handed out by uis_stream_commit (have + committed = received)
    int64_t log_len = 0;              // entries of st.logblk / st.logden
    std::vector<float> win_score;     // rank 0's score at the last commit: what an utterance whose window the commit emptied still has
    // everything committed, nothing received since: ONE hypothesis lives (all survivors shared the ancestor at the
    // last step), its labels are the committed ones and its score is win_score; the readouts' kernels see N = 0
    bool window_emptied(int u) const { return have[u] == 0 && committed[u] > 0; }
    std::vector<int32_t> limits;      // max_speakers per slot as the caller gave them (0: no bound): uis_stream_begin / uis_stream_limits
    // minimum turn length per slot as the caller gave them (0 and 1: no rule): uis_session_min_turn.  d_min_turn holds
    // them on the device; st.min_turn points there exactly while some slot has a value of 2 or more, else it is null
    std::vector<int32_t> min_turn;
    int32_t* d_min_turn = nullptr;
    DecodeState st{};
    int32_t* d_have = nullptr;        // frames received per utterance, refreshed for every back-trace
    int64_t* d_lab_off = nullptr;
    float* d_beam_scores = nullptr;
    // one-launch steps (k_decode_resident per push) where the shape allows it
    bool resident = false;
    bool coop_checked = false;        // one push of this session already went through the cooperative launch
    uint32_t* d_ctl = nullptr;
    size_t ctl_words = 0;
    // persistent launch (UIS_FLAG_PERSISTENT): k_decode_resident<.., true> stays on the device between
    // pushes; commands, tables, frames and labels travel through pm_block (host-coherent pinned memory)
    bool persist = false;             // the session asked for it and its shape allows it
    bool pm_running = false;          // the launch is on the device
    uint32_t pm_seq = 0;              // commands issued to the running launch
    MailboxLayout mailbox;            // where everything lies in pm_block, and each cluster's fixed share of the chunk's rows
    unsigned long long* d_go = nullptr;
    unsigned char* d_hdr = nullptr;
    PersistArgs pm_args{};            // host copy of what d_pm_args holds
    PersistArgs* d_pm_args = nullptr;
    int64_t pm_launches = 0;
    UisPoison poison;                 // UIS_POISON_WORKSPACE as uis_stream_begin / the running uis_stream_push read it
    // a push, a prime or an import has given the session a non-zero speaker tag (uis_stream_speakers): from then on, and
    // until uis_stream_end, no utterance may reach 2^24 frames received (the tag shares the block-count word)
    bool tagged = false;
  } stream_state;
  size_t dbg_floats = 0;  // what the last decode left in dbg_scores (UIS_FLAG_DEBUG_SCORES)
  UisPoison poison;  // UIS_POISON_WORKSPACE as the running uis_decode* call read it at its entry (one getenv per call)
  const double* const* src64 = nullptr;  // uis_decode_f64: the caller's float64 utterances (set for the duration of that call)
  void* cast_pool = nullptr;  // CastPool: the threads that cast (created by the first uis_decode_f64)
  ProfileEvents prof;
  hipEvent_t ev_begin = nullptr, ev_end = nullptr, ev_pre = nullptr;
  hipEvent_t ev_producer = nullptr;  // recorded on the caller's stream by the tensor entry points (created by the first of them)
  // utterance groups: one stream + one cached step graph each
  std::vector<hipStream_t> gstreams;
  std::vector<hipEvent_t> gdone;
  std::vector<GraphCache> gcache;
  // info of the last decode
  int last_U = 0, last_B = 0;
  KernelPick last_pick;  // the kernel-table entry behind the last decode / the last launch of a session push
  std::vector<int64_t> io_offsets;  // offsets of the last uis_decode (its labels are still in io_labels)
  std::vector<int32_t> last_overflow;
  std::vector<float> last_beam_scores;
  // the per-call input tables (max_speakers, per-frame transition_bias, known speakers of a decode and of a session's
  // calls): as their setters left them, and as the running call took them (uis_call_tables.h)
  CallTables tables;
  // n-best readout (uis_nbest.hip): what the last decode that returned UIS_OK / UIS_ERR_CLUSTER_CAP left behind --
  // every group's DecodeState (views into the workspace, which only the next decode rewrites), the utterances'
  // offsets, the record format
  struct NbestGroup { DecodeState st; int u0; };
  bool nb_valid = false, nb_wnd = false;
  int nb_B = 0;
  std::vector<NbestGroup> nb_groups;
  std::vector<int64_t> nb_offsets;
};

namespace {

static_assert(UIS_TAGGED_FRAMES_END == (int64_t)1 << UIS_BLK_TAG_SHIFT, "uis_call_tables.h restates the block-count word's tag shift");

// Every entry point that a table concerns opens with this: its rule over the handle's tables (uis_call_tables.h).  A
// null handle passes: the call's own check reports it.
int begin_call(uis_handle* h, const char* who, const TableRule& rule) {
  return h ? table_status(h->tables.begin(who, rule)) : UIS_OK;
}

inline volatile uint32_t* pm_ctl(uis_handle::Stream& ss) { return ss.pm_block.as<volatile uint32_t>(); }

// every cluster's doorbell: command words first, then the sequence numbers
void pm_ring(uis_handle::Stream& ss, uint32_t seq, uint32_t type, uint32_t frames, const uint32_t* row0 = nullptr,
             const uint32_t* nrow = nullptr) {
  volatile uint32_t* ctl = pm_ctl(ss);
  const int ncl = ss.st.ncl;
  for (int c = 0; c < ncl; ++c) {
    ctl[UIS_PM_BELL_WORD + 16 * c + 1] = type | (frames << 8);
    ctl[UIS_PM_BELL_WORD + 16 * c + 2] = row0 ? (row0[c] | (nrow[c] << 16)) : 0u;
    ctl[UIS_PM_BELL_WORD + 16 * c + 3] = seq;
  }
  std::atomic_thread_fence(std::memory_order_release);
  for (int c = 0; c < ncl; ++c) ctl[UIS_PM_BELL_WORD + 16 * c] = seq;
  std::atomic_thread_fence(std::memory_order_seq_cst);
}

// Where hidden unit j of the model sits in the padded hidden vector (round 6).  Padding a hidden size up to a kernel's
// shape is exact only if every canonical K segment (uis_numerics.h: q = ceil(blocks / 8) k-blocks each) keeps its
// blocks: appending zeros does that where q is the kernel's (q 1 -> 128, 2 -> 256, 4 -> 512), and for q = 3 (hidden sizes
// 257 .. 384) the zeros go INSIDE: segment s's three blocks into the first three of the kernel's four
// (unit j -> (j / 48) * 64 + j % 48), a zero block behind each.  fma(0, 0, acc) = acc: no bit moves, every sum keeps
// its association, and the units in between stay exactly 0 (zero weights and biases: gates 1/2, candidate 0, h' = h / 2 = 0).
struct HidMap {
  int seg = 0, seg_p = 0;  // floats per canonical segment of the model / of the kernel's shape (0: identity)
  int operator()(int j) const { return seg ? (j / seg) * seg_p + j % seg : j; }
};

// Re-pack a (n_out x K) row-major matrix (optionally 3 stacked gates of `rows_per_gate`
// rows each, padded to `rows_per_gate_p`) into MFMA tile order:
//   out[((tile*nKb + kb)*64 + lane)*4 + r] = W[tile*16 + (lane&15)][kb*16 + 4*(lane>>4) + r]
// rmap / kmap: where a row (within its gate) / a column goes in the padded layout (the hidden axis: HidMap).
std::vector<float> tile_weights(const float* W, int gates, int rows_per_gate, int rows_per_gate_p, int K, int Kp,
                                HidMap rmap = HidMap(), HidMap kmap = HidMap()) {
  const int Fp = gates * rows_per_gate_p;
  const int nKb = Kp / 16;
  std::vector<float> out((size_t)Fp * Kp, 0.0f);
  for (int g = 0; g < gates; ++g)
    for (int j = 0; j < rows_per_gate; ++j) {
      const int fp = g * rows_per_gate_p + rmap(j), tile = fp / 16;
      const float* src = W + (size_t)(g * rows_per_gate + j) * K;
      for (int k = 0; k < K; ++k) {
        const int kp = kmap(k), kb = kp / 16, q = (kp % 16) / 4, r = kp % 4;
        out[(((size_t)tile * nKb + kb) * 64 + (q * 16 + fp % 16)) * 4 + r] = src[k];
      }
    }
  return out;
}

std::vector<float> pad_bias(const float* b, int gates, int n, int np, HidMap map = HidMap()) {
  std::vector<float> out((size_t)gates * np, 0.0f);
  for (int g = 0; g < gates; ++g)
    for (int j = 0; j < n; ++j) out[(size_t)g * np + map(j)] = b[(size_t)g * n + j];
  return out;
}

int upload(uis_handle* h, const std::vector<float>& v, const float** dst) {
  void* p = nullptr;
  HIPCHK(hipMalloc(&p, std::max<size_t>(v.size(), 4) * sizeof(float)));
  h->model_allocs.push_back(p);
  HIPCHK(hipMemcpy(p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
  *dst = reinterpret_cast<const float*>(p);
  return UIS_OK;
}

#define UIS_PROJ_WIDE_ROWS 2048  // frames from which the input projection runs its 2 x 4-tile-per-wave kernel
inline dim3 dense_grid(long rows, int tiles) { return dim3((unsigned)((rows + 15) / 16), (unsigned)((tiles + 3) / 4), 1); }
// 1-D, XCD-aware grid of the per-step dense kernels (dense_block_map in uis_kernels.hip)
inline dim3 dense_grid_xcd(long rows, int tiles) {
  return dim3((unsigned)dense_grid_blocks((int)((rows + 15) / 16), tiles), 1, 1);
}

// Events of a vector that only grows (one per copy piece, group, profiled launch): create until there are n.
int grow_events(std::vector<hipEvent_t>& ev, size_t n, unsigned flags = hipEventDisableTiming) {
  while (ev.size() < n) {
    hipEvent_t e;
    HIPCHK(hipEventCreateWithFlags(&e, flags));
    ev.push_back(e);
  }
  return UIS_OK;
}

// Launches go through here.  With UIS_FLAG_PROFILE every kernel is launched with
// hipExtLaunchKernelGGL's start/stop events, which carry the dispatch's own begin/end
// timestamps (what rocprofv3 --kernel-trace reports), not host-side bracket times.
struct Launcher {
  uis_handle* h;
  hipStream_t stream;
  bool profile;
  int events(hipEvent_t* a, hipEvent_t* b, int cls) {
    ProfileEvents& p = h->prof;
    if (int rc = grow_events(p.ev, p.used + 2, hipEventDefault)) return rc;
    p.cls.push_back(cls);
    *a = p.ev[p.used];
    *b = p.ev[p.used + 1];
    p.used += 2;
    return UIS_OK;
  }
  template <typename... KArgs, typename... Args>
  int run(int cls, void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t shmem, Args... args) {
    if (profile) {
      hipEvent_t a, b;
      int rc = events(&a, &b, cls);
      if (rc) return rc;
      hipExtLaunchKernelGGL(kernel, grid, block, shmem, stream, a, b, 0, args...);
    } else {
      hipLaunchKernelGGL(kernel, grid, block, shmem, stream, args...);
    }
    HIPCHK(hipGetLastError());
    return UIS_OK;
  }
  // The one-launch decode spins on in-launch barriers: every workgroup of the grid must be
  // resident at once.  hipLaunchCooperativeKernel guarantees that (or refuses the launch); the
  // occupancy query is checked as well so that the refusal has a readable reason.  With
  // `profile`, events recorded around the launch on the same (otherwise idle) stream.
  // `cooperative` = false: a plain launch of the same grid after the occupancy check (same
  // residency, 15-19 us less host time per launch: MI355X_MICROARCH.md "coop-launch"); used by the
  // streaming pushes after the session's first push went through the cooperative path.
  template <typename... KArgs>
  int run_cooperative(int cls, void (*kernel)(KArgs...), int n_cu, dim3 grid, dim3 block, size_t shmem, bool cooperative,
                      KArgs... args) {
    int per_cu = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(kernel), (int)block.x, shmem));
    if ((long)per_cu * n_cu < (long)grid.x) {
      h->inlaunch_failed = true;
      return fail(UIS_ERR_HIP, "one-launch decode: " + std::to_string(grid.x) + " workgroups cannot be co-resident (" +
                                   std::to_string(per_cu) + " per CU x " + std::to_string(n_cu) + " CUs)");
    }
    hipEvent_t a = nullptr, b = nullptr;
    if (profile) {
      int rc = events(&a, &b, cls);
      if (rc) return rc;
      HIPCHK(hipEventRecord(a, stream));
    }
    void* argv[] = {static_cast<void*>(&args)...};
    hipError_t e;
    if (cooperative) {
      e = hipLaunchCooperativeKernel(reinterpret_cast<const void*>(kernel), grid, block, argv, (unsigned)shmem, stream);
    } else {
      hipLaunchKernelGGL(kernel, grid, block, shmem, stream, args...);
      e = hipGetLastError();
    }
    if (e != hipSuccess) {
      (void)hipGetLastError();
      h->inlaunch_failed = true;  // the caller falls back to the launch-per-step path
      return fail(UIS_ERR_HIP, std::string("hipLaunchCooperativeKernel(k_decode_resident): ") + hipGetErrorString(e));
    }
    if (profile) HIPCHK(hipEventRecord(b, stream));
    return UIS_OK;
  }
};

#define LAUNCH(...)                       \
  do {                                    \
    int rc_ = lch.run(__VA_ARGS__);       \
    if (rc_) return rc_;                  \
  } while (0)

// The input projection of n frames with the plain kernels: gi0 = W_ih0 x + b_ih0, then mse0.
int plain_input_proj(Launcher& lch, const DevModel& m, const float* x, float* gi0, float* mse0, long n) {
  LAUNCH(UIS_K_INPUT_PROJ, k_dense_input_proj, dense_grid(n, m.G / 16), dim3(256), 0, m, x, gi0, n);
  LAUNCH(UIS_K_INPUT_PROJ, k_mse0, dim3((unsigned)((n + 3) / 4)), dim3(256), (size_t)5 * m.Dp * 4, m, x, mse0, n, 0L, (const long*)nullptr);
  return UIS_OK;
}

// One batched CoreRNN evaluation over the rows emitted for step parity `par`.
// Which family of dense kernels the launch-per-step path runs for a step of at most `max_rows`
// rnn rows (UIS_DF_*; uis_stats.decode_kernel reports it).
int dense_family(const DevModel& m, int n_cu, uint32_t flags, long max_rows) {
  if (max_rows > UIS_WT_ROWS && (m.Hp == 512 || m.Hp == 256) && m.Dp % 16 == 0 && !(flags & UIS_FLAG_SMALL_TILES) && n_cu >= 64)
    return UIS_DF_WT;
  if (max_rows > UIS_WIDE_TILE_ROWS && (m.Hp / 16) % 4 == 0 && (m.Dp / 16) % 4 == 0 && !(flags & UIS_FLAG_SMALL_TILES))
    return UIS_DF_BIG;
  return UIS_DF_DENSE;
}

int launch_rnn(uis_handle* h, Launcher& lch, const DecodeState& st, int par, long max_rows) {
  const DevModel& m = h->m;
  const int mr = (int)max_rows;
  const bool wide = max_rows > UIS_WIDE_TILE_ROWS;  // tile shape, see uis_kernels.hip
  const int family = dense_family(m, h->n_cu, st.flags, max_rows);
  // thousands of rows: the big-tile kernels (4 row tiles x several feature tiles per workgroup,
  // full-K chains per wave) where the feature-tile counts divide
  // thousands of rows and hidden size 256 / 512: weights in LDS, a wave per row tile (k_wt_*)
  // (measured crossover against the 1x1 split-K tiles: row capacity 1280 about equal, 1920 +11 %)
  if (family == UIS_DF_WT) {
    const int nft = m.Hp / 16, nft2 = m.Dp / 16;
    const int ng1 = wt_groups(h->n_cu, nft);
    const size_t kb_bytes = (size_t)nft * 1024;  // one weight stream of a feature tile: all k-blocks
    for (int l = 0; l < m.depth; ++l) {
      // (layers >= 1: the input-side gates by the same kernel, W_ih in the LDS slot; UIS_WT_NO_UPPER=1 keeps the split-K tiles)
      static const bool wt_upper = getenv("UIS_WT_NO_UPPER") == nullptr;
      if (l > 0 && !wt_upper) LAUNCH(UIS_K_UPPER_IN, k_dense_upper_in, dim3(step_grid_blocks(mr, m.G / 16, 1, 1)), dim3(512), 0, m, st, par, l);
      if (l > 0 && wt_upper && m.Hp == 512) LAUNCH(UIS_K_UPPER_IN, (k_wt_gru<32, true>), dim3(nft * ng1), dim3(512), 3 * kb_bytes, m, st, par, l, ng1);
      if (l > 0 && wt_upper && m.Hp != 512) LAUNCH(UIS_K_UPPER_IN, (k_wt_gru<16, true>), dim3(nft * ng1), dim3(512), 3 * kb_bytes, m, st, par, l, ng1);
      if (m.Hp == 512) LAUNCH(UIS_K_GRU, k_wt_gru<32>, dim3(nft * ng1), dim3(512), 3 * kb_bytes, m, st, par, l, ng1);
      else LAUNCH(UIS_K_GRU, k_wt_gru<16>, dim3(nft * ng1), dim3(512), 3 * kb_bytes, m, st, par, l, ng1);
    }
    // two feature tiles per workgroup of the heads where the tile count is even (measured on
    // configs[2]: one 66.4 / 36.7 ms per pass for the two heads, two 49.0 / 30.9, four 55.1 / 39.4)
    const int na1 = nft % 2 == 0 ? 2 : 1, na2 = nft2 % 2 == 0 ? 2 : 1;
    const int nh1 = wt_groups(h->n_cu, nft / na1), nh2 = wt_groups(h->n_cu, nft2 / na2);
#define UIS_WT_HEAD(NKB_, HEAD_, NA_, tiles_, ng_) \
  LAUNCH(HEAD_ == 1 ? UIS_K_HEAD1 : UIS_K_HEAD2, (k_wt_head<NKB_, HEAD_, NA_>), dim3((tiles_) / NA_ * (ng_)), dim3(512), NA_ * kb_bytes, m, st, par, ng_)
    if (m.Hp == 512) {
      if (na1 == 2) UIS_WT_HEAD(32, 1, 2, nft, nh1); else UIS_WT_HEAD(32, 1, 1, nft, nh1);
      if (na2 == 2) UIS_WT_HEAD(32, 2, 2, nft2, nh2); else UIS_WT_HEAD(32, 2, 1, nft2, nh2);
    } else {
      if (na1 == 2) UIS_WT_HEAD(16, 1, 2, nft, nh1); else UIS_WT_HEAD(16, 1, 1, nft, nh1);
      if (na2 == 2) UIS_WT_HEAD(16, 2, 2, nft2, nh2); else UIS_WT_HEAD(16, 2, 1, nft2, nh2);
    }
#undef UIS_WT_HEAD
    return UIS_OK;
  }
  if (family == UIS_DF_BIG) {
    for (int l = 0; l < m.depth; ++l) {
      if (l > 0) LAUNCH(UIS_K_UPPER_IN, k_dense_upper_in, dim3(step_grid_blocks(mr, m.G / 16, 1, 1)), dim3(512), 0, m, st, par, l);
      LAUNCH(UIS_K_GRU, k_big_gru<2>, dim3(big_grid_blocks(mr, m.Hp / 16, 2)), dim3(256), 0, m, st, par, l);
    }
    LAUNCH(UIS_K_HEAD1, k_big_head1<4>, dim3(big_grid_blocks(mr, m.Hp / 16, 4)), dim3(256), 0, m, st, par);
    LAUNCH(UIS_K_HEAD2, k_big_head2<4>, dim3(big_grid_blocks(mr, m.Dp / 16, 4)), dim3(256), 0, m, st, par);
    return UIS_OK;
  }
  for (int l = 0; l < m.depth; ++l) {
    if (l > 0) LAUNCH(UIS_K_UPPER_IN, k_dense_upper_in, dim3(step_grid_blocks(mr, m.G / 16, 1, 1)), dim3(512), 0, m, st, par, l);
    if (wide) LAUNCH(UIS_K_GRU, k_dense_gru<2>, dim3(step_grid_blocks(mr, m.Hp / 16, 2, 1)), dim3(512), 0, m, st, par, l);
    else LAUNCH(UIS_K_GRU, k_dense_gru<1>, dim3(step_grid_blocks(mr, m.Hp / 16, 1, 1)), dim3(512), 0, m, st, par, l);
  }
  if (wide) {
    LAUNCH(UIS_K_HEAD1, (k_dense_head1<2, 2>), dim3(step_grid_blocks(mr, m.Hp / 16, 2, 2)), dim3(512), 0, m, st, par);
    LAUNCH(UIS_K_HEAD2, k_dense_head2<2>, dim3(step_grid_blocks(mr, m.Dp / 16, 2, 1)), dim3(512), 0, m, st, par);
  } else {
    LAUNCH(UIS_K_HEAD1, (k_dense_head1<1, 1>), dim3(step_grid_blocks(mr, m.Hp / 16, 1, 1)), dim3(512), 0, m, st, par);
    LAUNCH(UIS_K_HEAD2, k_dense_head2<1>, dim3(step_grid_blocks(mr, m.Dp / 16, 1, 1)), dim3(512), 0, m, st, par);
  }
  return UIS_OK;
}

// One CoreRNN.forward (uisrnn.py:45-52) of a single row with the decode kernels themselves:
// x [Dp] and h_in [depth][Hp] on the device -> mean [Dp], h_out [depth][Hp] on the device.
int rnn_step_once(uis_handle* h, const float* d_x, const float* d_hin, float* d_mean, float* d_hout) {
  DevModel& m = h->m;
  Launcher lch{h, h->stream, false};
  float *d_gi0 = nullptr, *d_gi_up = nullptr, *d_a1 = nullptr;
  RnnRow* d_rows = nullptr;
  int32_t* d_nrows = nullptr;
  Scratch tmp;
  int rc;
  if ((rc = tmp.get(&d_gi0, (size_t)m.G)) || (rc = tmp.get(&d_gi_up, (size_t)64 * m.G)) ||
      (rc = tmp.get(&d_a1, (size_t)64 * m.Hp)) || (rc = tmp.get(&d_rows, 64)) || (rc = tmp.get(&d_nrows, 2)))
    return rc;
  HIPCHK(hipMemsetAsync(d_rows, 0, 64 * sizeof(RnnRow), h->stream));
  HIPCHK(hipMemsetAsync(d_a1, 0, 64 * m.Hp * sizeof(float), h->stream));
  RnnRow rr{};
  rr.utt = 0; rr.src = -1; rr.dst = 0; rr.nprev = 0; rr.frame = 0;
  int32_t nr[2] = {1, 1};
  HIPCHK(hipMemcpyAsync(d_rows, &rr, sizeof(rr), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(d_nrows, nr, sizeof(nr), hipMemcpyHostToDevice, h->stream));
  LAUNCH(UIS_K_INPUT_PROJ, k_dense_input_proj, dense_grid(1, m.G / 16), dim3(256), 0, m, d_x, d_gi0, 1L);
  DecodeState st{};
  st.U = 1; st.B = 1; st.Kmax = 1; st.S = 1; st.L = 1; st.tau = 1; st.max_rows = 1;
  st.gi0 = d_gi0; st.pool_mean = d_mean; st.pool_hid = d_hout; st.rows = d_rows; st.nrows = d_nrows;
  st.gi_up = d_gi_up; st.a1 = d_a1;
  const float* saved_h1 = m.h1;
  m.h1 = d_hin;  // a row with src = -1 reads its hidden state from "h1": point that at h_in
  rc = launch_rnn(h, lch, st, 0, 1);
  m.h1 = saved_h1;
  hipError_t se = hipStreamSynchronize(h->stream);  // before `tmp` frees what the kernels use
  if (rc) return rc;
  HIPCHK(se);
  return UIS_OK;
}

// (m0, h1) = CoreRNN(0, rnn_init_hidden)  (uisrnn.py:435-439).
int bootstrap_constants(uis_handle* h, const float* d_hinit) {
  DevModel& m = h->m;
  float *d_x = nullptr, *d_pm = nullptr, *d_ph = nullptr;
  const size_t hid_elems = (size_t)m.depth * m.Hp;
  Scratch tmp;
  int rc;
  if ((rc = tmp.get(&d_x, (size_t)m.Dp)) || (rc = tmp.get(&d_pm, (size_t)m.Dp)) || (rc = tmp.get(&d_ph, hid_elems))) return rc;
  HIPCHK(hipMemsetAsync(d_x, 0, m.Dp * sizeof(float), h->stream));
  if ((rc = rnn_step_once(h, d_x, d_hinit, d_pm, d_ph))) return rc;
  HIPCHK(hipMemcpy(const_cast<float*>(m.m0), d_pm, m.Dp * sizeof(float), hipMemcpyDeviceToDevice));
  HIPCHK(hipMemcpy(const_cast<float*>(m.h1), d_ph, hid_elems * sizeof(float), hipMemcpyDeviceToDevice));
  return UIS_OK;
}

// Everything one utterance group needs: a view of the shared buffers (pointers offset to
// the group's first utterance), its stream and its captured step graph.
struct GroupPlan {
  int u0 = 0, U = 0;
  int64_t maxT = 0;
  DecodeState st{};
};

// The kernels of `nsteps` consecutive decode steps (starting at an even step) on `stream`.
int enqueue_steps(uis_handle* h, Launcher& lch, const DecodeState& st, size_t select_lds, int nsteps) {
  const DevModel& m = h->m;
  const long max_rows = st.max_rows;
  for (int s = 0; s < nsteps; ++s) {
    const int par = s & 1;
    if (!st.wnd && select_fast_ok(st.B, st.Kmax, st.S) && !(st.flags & UIS_FLAG_GENERIC_SELECT))
      LAUNCH(UIS_K_SELECT, k_select_fast, dim3(st.U), dim3(256), (size_t)fast_lds_layout(m.Dp, st.B, st.Kmax, st.S).total, m, st, par);
    else if (!st.wnd) LAUNCH(UIS_K_SELECT, k_select, dim3(st.U), dim3(256), select_lds, m, st, par);
    else if (st.NC >= UIS_WINDOW_WIDE_LEVEL)  // hundreds of hypotheses per level: more threads per utterance
      LAUNCH(UIS_K_EXPAND, k_window<UIS_WINDOW_WIDE_NT>, dim3(st.U), dim3(UIS_WINDOW_WIDE_NT), window_lds_bytes(window_scratch_layout(st.S, st.NC, st.Kmax, st.B)), m, st, par);
    else LAUNCH(UIS_K_EXPAND, k_window<256>, dim3(st.U), dim3(256), window_lds_bytes(window_scratch_layout(st.S, st.NC, st.Kmax, st.B)), m, st, par);
    int rc = launch_rnn(h, lch, st, par, max_rows);
    if (rc) return rc;
  }
  return UIS_OK;
}

// float64 -> float32 of the packed frame matrix, read from the caller's per-utterance arrays (the
// reference casts once with torch's .float(), round to nearest even, uisrnn/uisrnn.py:524-526; so
// does a C++ double -> float conversion), by a few host threads -- one team for a whole decode:
// the threads are started once and take blocks of rows in order; the caller asks for a prefix of the
// rows (`wait_rows`), helping with blocks while it waits, and hands each finished piece to the copy
// engine while the team is already in the next.
static bool agent_flags_env() {  // UIS_AGENT_FLAGS=1: the conforming phase-word stores (UIS_FLAG_AGENT_FLAGS) for every decode of the process
  static const bool v = getenv("UIS_AGENT_FLAGS") != nullptr && atoi(getenv("UIS_AGENT_FLAGS")) != 0;
  return v;
}
static bool getenv_flag_no_stream() {  // UIS_CAST_PLAIN_STORES=1: the scalar loop with ordinary stores (A/B)
  static const bool v = getenv("UIS_CAST_PLAIN_STORES") != nullptr;
  return v;
}
struct CastTeam {
  static constexpr int64_t kBlockRows = 512;
  const double* const* utt; const int64_t* offsets; int n_utt, D; int64_t F; float* dst;
  int64_t nblocks = 0;
  std::atomic<int64_t> next{0};
  std::vector<std::atomic<unsigned char>> done;
  // (round 5) `order`, if given: the row ranges to cast, in this order, instead of the packed matrix front to back --
  // the first frames of EVERY utterance before the later ones, when a decode starts on a time slice
  std::vector<std::pair<int64_t, int64_t>> order;
  // ... and `dst_rows`, if given: where block b's first row goes in the staging block (a ragged list's slices are laid
  // out slice after slice, so that a slice is ONE copy); without it a row keeps its place in the packed matrix
  std::vector<int64_t> dst_rows;
  CastTeam(const double* const* utt_, const int64_t* offsets_, int n_utt_, int D_, int64_t F_, float* dst_,
           std::vector<std::pair<int64_t, int64_t>> order_ = {}, std::vector<int64_t> dst_rows_ = {})
      : utt(utt_), offsets(offsets_), n_utt(n_utt_), D(D_), F(F_), dst(dst_),
        nblocks(order_.empty() ? (F_ + kBlockRows - 1) / kBlockRows : (int64_t)order_.size()),
        done((size_t)(order_.empty() ? (F_ + kBlockRows - 1) / kBlockRows : (int64_t)order_.size())), order(std::move(order_)),
        dst_rows(std::move(dst_rows_)) {
    for (auto& d : done) d.store(0, std::memory_order_relaxed);
  }
  void wait_blocks(int64_t b1) {  // blocks [0, b1) of `order` are cast when this returns
    for (int64_t b = 0; b < b1; ++b)
      while (!done[(size_t)b].load(std::memory_order_acquire))
        if (!take()) std::this_thread::yield();
  }
  // how many threads are worth waking: >= 1 MB of input each
  unsigned want_threads(unsigned have) const {
    return (unsigned)std::min<int64_t>(have, std::max<int64_t>(1, F * D / (1 << 17)));
  }
  bool take() {  // one block, if there is one left
    const int64_t b = next.fetch_add(1, std::memory_order_relaxed);
    if (b >= nblocks) return false;
    if (order.empty()) cast_block(b * kBlockRows, std::min(F, (b + 1) * kBlockRows), -1);
    else cast_block(order[(size_t)b].first, order[(size_t)b].second, dst_rows.empty() ? -1 : dst_rows[(size_t)b]);
#if defined(UIS_HOST_SSE2)
    _mm_sfence();  // (the streaming stores above are ordered before the flag)
#endif
    done[(size_t)b].store(1, std::memory_order_release);
    return true;
  }
  void cast_block(int64_t r0, int64_t r1, int64_t drow) {  // (drow >= 0: row r0 goes to row drow of the staging block)
    int u = (int)(std::upper_bound(offsets, offsets + n_utt + 1, r0) - offsets) - 1;  // the utterance holding row r0
    for (int64_t r = r0; r < r1;) {
      while (offsets[u + 1] <= r) ++u;  // (empty utterances)
      const int64_t e = std::min(r1, offsets[u + 1]);
      const double* src = utt[u] + (size_t)(r - offsets[u]) * D;
      float* d = dst + (size_t)(drow >= 0 ? drow + (r - r0) : r) * D;
      const int64_t n = (e - r) * D;
      int64_t i = 0;
#if defined(UIS_HOST_SSE2)
      // four values per step, written around the cache (cvtpd2ps rounds like the scalar conversion: MXCSR,
      // to nearest even): the float32 block is read next by the copy engine, not by this core, and an
      // ordinary store would first fetch every destination line -- a third more DRAM traffic on the
      // NUMA node that bounds this loop
      if (!getenv_flag_no_stream()) {
        while (i < n && (reinterpret_cast<uintptr_t>(d + i) & 15u)) { d[i] = (float)src[i]; ++i; }
        for (; i + 4 <= n; i += 4) {
          const __m128 lo = _mm_cvtpd_ps(_mm_loadu_pd(src + i)), hi = _mm_cvtpd_ps(_mm_loadu_pd(src + i + 2));
          _mm_stream_ps(d + i, _mm_movelh_ps(lo, hi));
        }
      }
#endif
      for (; i < n; ++i) d[i] = (float)src[i];
      r = e;
    }
  }
  void wait_rows(int64_t f1) { wait_blocks((f1 + kBlockRows - 1) / kBlockRows); }  // rows [0, f1) are cast when this returns
};

// The threads that cast: created once per handle (a decode used to spawn and join up to sixteen
// std::threads of its own -- a third of a millisecond before the first block was cast), asleep on a
// condition variable between decodes.  They follow the affinity mask of the thread that created the
// pool (bench.py pins a rank to its share of the cores first).
struct CastPool {
  std::vector<std::thread> threads;
  std::mutex mu;
  std::condition_variable cv_work, cv_idle;
  CastTeam* job = nullptr;
  uint64_t generation = 0;
  unsigned wanted = 0, busy = 0;
  bool quit = false;
  void ensure_started() {
    if (!threads.empty() || quit) return;
    // (measured on the 256-core GPU box, configs[1], frames/s of the float64 leg: 4 / 8 threads 1.600 M, 16 1.56-1.59 M,
    // 24 1.59 M, 32 1.58 M, 48 1.59 M -- the cast is a few hundred microseconds of memory traffic; more threads only
    // add wake-up jitter: profiles/r04_f64_leg.txt)
    unsigned nt = std::min(std::max(1u, std::thread::hardware_concurrency()), 8u);
    if (const char* e = getenv("UIS_CAST_THREADS")) nt = (unsigned)std::max(1, atoi(e));
    try {
      for (unsigned k = 1; k < nt; ++k) threads.emplace_back([this, k]() { worker(k); });
    } catch (...) {  // no more threads to be had: the caller's thread does what is left (CastTeam::wait_rows)
    }
  }
  void worker(unsigned index) {
    uint64_t seen = 0;
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv_work.wait(lk, [&]() { return quit || generation != seen; });
      if (quit) return;
      seen = generation;
      CastTeam* j = job;
      if (!j || index > wanted) continue;
      ++busy;
      lk.unlock();
      while (j->take()) {}
      lk.lock();
      if (--busy == 0) cv_idle.notify_all();
    }
  }
  void post(CastTeam* j) {
    ensure_started();
    std::lock_guard<std::mutex> lk(mu);
    job = j;
    wanted = j->want_threads((unsigned)threads.size() + 1) - 1;  // (the caller's thread is one of the team)
    ++generation;
    cv_work.notify_all();
  }
  void finish() {  // the job is about to go out of scope: nobody may still be inside it
    std::unique_lock<std::mutex> lk(mu);
    job = nullptr;
    cv_idle.wait(lk, [&]() { return busy == 0; });
  }
  ~CastPool() {
    {
      std::lock_guard<std::mutex> lk(mu);
      quit = true;
      job = nullptr;
    }
    cv_work.notify_all();
    for (auto& th : threads) th.join();
  }
};

// ---- which kernels decode a list: plan_decode() decides, decode_once() carries the plan out

// The environment switches the decode path honours, read once per decode, at the top of decode_once (tests change
// os.environ between calls).
//   UIS_MAX_STATE_BYTES   a smaller ceiling on the decode state, for tests of the host layer's answer (halving)
//   UIS_SPLIT_MIN_MB      list size from which a host list is decoded in slices (tests, experiments)
//   UIS_SPLIT_FRAMES      a,b,..: the slice boundaries instead of the library's schedule
//   UIS_NO_SPLIT          one launch (A/B switch, bit-identical)
//   UIS_NO_ARENA, UIS_ARENA_SHIFT, UIS_NO_CTL_TUNE, UIS_CTL_OFFSET   buffer placement (tools/experiments/bimodal.py)
//   UIS_AGENT_FLAGS       (read once per process) UIS_FLAG_AGENT_FLAGS on every decode
//   UIS_POISON_WORKSPACE  a 32-bit hex word: every call fills the working memory it is about to use with it before its first
//                         write (uis_poison.h; also read, once per call, by the sessions, the readouts, uis_score_labels,
//                         uis_eval_* and uis_train_step).  A test switch: no output may depend on stale memory
struct DecodeKnobs {
  double max_state_bytes = 200e9, split_min_bytes = 0.0;
  bool split_min_set = false, split_frames_set = false, no_split = false, no_arena = false, no_ctl_tune = false;
  bool ctl_offset_set = false, agent_flags = false;
  bool no_rs = false;  // (not from the environment: plan_and_place sets it when k_decode_rs's workspace stretch would pass 4 GB)
  std::vector<long> split_frames;
  size_t arena_shift = 0, ctl_offset = 0;
};

DecodeKnobs read_knobs() {
  DecodeKnobs k;
  if (const char* e = getenv("UIS_MAX_STATE_BYTES")) k.max_state_bytes = atof(e);
  if (const char* e = getenv("UIS_SPLIT_MIN_MB")) { k.split_min_set = true; k.split_min_bytes = 1e6 * atof(e); }
  if (const char* e = getenv("UIS_SPLIT_FRAMES")) {
    k.split_frames_set = true;
    for (const char* p = e; *p;) {
      char* end = nullptr;
      const long v = strtol(p, &end, 10);
      if (end == p) break;
      k.split_frames.push_back(v);
      p = *end ? end + 1 : end;
    }
  }
  k.no_split = getenv("UIS_NO_SPLIT") != nullptr;
  k.no_arena = getenv("UIS_NO_ARENA") != nullptr;
  if (const char* e = getenv("UIS_ARENA_SHIFT")) k.arena_shift = (size_t)atol(e) & ~(size_t)4095;
  k.no_ctl_tune = getenv("UIS_NO_CTL_TUNE") != nullptr;
  if (const char* e = getenv("UIS_CTL_OFFSET")) { k.ctl_offset_set = true; k.ctl_offset = (size_t)atol(e) & ~(size_t)127; }
  k.agent_flags = agent_flags_env();
  return k;
}

// What the planner needs to know about a decode besides the model.
struct DecodeShape {
  int U, G, B, Kmax, L, S;     // utterances, utterance groups (streams), beam, cluster cap, look_ahead, slots per utterance
  int64_t F, maxN, maxT, NC;   // frames, longest utterance, its steps (test_iteration x), level capacity
  bool ragged;                 // utterances of different lengths
  bool f64;                    // uis_decode_f64: float64 utterances, cast by the library
  bool host_frames;            // the frames are in host memory (uis_decode / uis_decode_f64)
  bool wnd;                    // the window machinery decodes (look_ahead >= 2, wide beams, select tables beyond LDS)
  size_t select_lds;           // select_lds_layout(...).total (without wnd)
  size_t window_scratch;       // window_scratch_layout(...).total
  // the call has a per-frame transition_bias table (uis_frame_bias).  k_decode_rs and k_decode_big<WS> form their priors
  // in rs_prep, which knows no table: such a decode runs the kernels with the owner-side selects
  bool biased = false;
  // the call has a per-frame speaker table (uis_frame_speakers).  The bindings ride in the block-count words, which the
  // replicated selects of k_decode_rs and k_decode_big<WS> keep in a layout of their own: excluded like `biased`
  // 
  bool hinted = false;
  // the call has a minimum turn length of 2 or more for some utterance (uis_min_turn).  The runs ride in the
  // last-label words, which those two kernels' selects likewise keep in a layout of their own: excluded like `biased`
  // 
  bool turned = false;
};

enum class DecodePath { STEPWISE, GRAPH, RESIDENT, RS, BIG, BIG_WS, WINDOW, DEEP, SMALL };
// the shapes of BASELINE's configs as compile-time constants
enum { CLS_NONE = 0, CLS_C1 /* configs[1] / [3]: beam 10, cap 16 */, CLS_C4 /* configs[4]: beam 20, cap 11 */,
       CLS_C2 /* configs[2]: beam 50, cap 12, look_ahead 2 */ };
// k_decode_rs's instantiations (uis_stats.decode_kernel bits 16..23; 3 .. 6 are reserved):
//   RS_BASE   beam_size <= 16, <= 192 candidates, observation dim <= 256, at most 8 utterances per XCD
//   RS_C1     ... with beam_size 10 / max_clusters 16 as compile-time constants (BASELINE configs[1])
enum { RS_NONE = 0, RS_BASE, RS_C1 };

// Where the one-launch kernels put their rows: the CUs form ncl clusters of 32 (one per XCD: 8 on a whole MI355X, 1 in
// CPX mode); one row region per cluster of rx_stride rows, a multiple of 16 (rows an utterance can emit per step:
// beam_size, or a level's capacity inside a look-ahead window) plus `slack`; rows_cap rows in all.
struct ClusterGeometry {
  int ncl = 0, nclq = 1;  // clusters of 32 CUs (0: the device has none), and at least 1
  int rx_stride = 0;      // rows of one cluster's row region
  long rows_cap = 0;
};

struct DecodePlan : ClusterGeometry {  // (the geometry the workspace shares with the choice)
  DecodePath path = DecodePath::STEPWISE;
  int rs_kind = RS_NONE;
  int cls = CLS_NONE;     // the shape class of the instantiation that runs (CLS_*)
  size_t lds = 0;         // dynamic LDS bytes of the decode kernel (stepwise: of the select)
  int decode_kernel = 0;  // uis_stats.decode_kernel
  bool split = false;     // several launches, the later frames travelling behind the earlier launches ...
  std::vector<int64_t> cuts;  // ... at these frame indices (empty without split)
  long max_rows = 0;
  bool hst = false;       // rnn_depth >= 2 at the cluster kernels' shapes: k_decode_deep's hand-off buffers
  bool stage = false;     // a ragged float64 list big enough to split: the device's copy of the staging block
  bool resident() const { return path == DecodePath::RESIDENT || path == DecodePath::RS || path == DecodePath::BIG || path == DecodePath::BIG_WS; }
  bool clustered() const { return resident() || path == DecodePath::WINDOW || path == DecodePath::DEEP; }
  bool one_launch() const { return clustered() || path == DecodePath::SMALL; }
};

ClusterGeometry cluster_geometry(int n_cu, int U, long rows_per_utt, int slack, int G) {
  ClusterGeometry g;
  g.ncl = (n_cu >= 32 && n_cu % 32 == 0 && n_cu / 32 <= UIS_MAX_CLUSTERS) ? n_cu / 32 : 0;
  g.nclq = std::max(g.ncl, 1);
  g.rx_stride = (int)(((((long)U + g.nclq - 1) / g.nclq) * rows_per_utt + 15) / 16 * 16) + slack;
  g.rows_cap = std::max((long)U * rows_per_utt + 48L * G, (long)g.nclq * g.rx_stride);  // every group's last row tile may run past its rows
  return g;
}

// What a one-launch decode with register-resident weights (k_decode_resident and its relatives) needs, before the
// callers' own terms: rnn_depth 1 at the instantiated dims, the fast select, a cluster, 2 GB descriptors, the LDS budget.
bool resident_fits(const DevModel& m, int U, int B, int Kmax, int S, const ClusterGeometry& g) {
  return m.depth == 1 && (m.Hp == 128 || m.Hp == 256 || m.Hp == 512) && (m.Dp == 128 || m.Dp == 256 || m.Dp == 512) &&
         select_fast_ok(B, Kmax, S) && g.ncl >= 1 && ((double)U * S + 1) * m.Hp * 4.0 < 2.0e9 &&
         (double)g.rows_cap * m.Hp * 4.0 < 2.0e9 && (double)U * S * m.Dp * 4.0 < 2.0e9 &&
         resident_lds_bytes(m.Hp, m.Dp, B, Kmax, S) <= 160 * 1024;
}

// The dynamic LDS of a one-launch kernel: at least 96 KB, so that a CU holds one workgroup.
size_t one_launch_lds(size_t lds) { return std::max<size_t>(lds, 96 * 1024); }

// The dispatch rule.  No HIP call, no allocation, no global state: the same inputs give the same plan.
DecodePlan plan_decode(const DevModel& m, const DecodeShape& s, uint32_t flags, const DecodeKnobs& k, int n_cu,
                       bool resident_off) {
  DecodePlan p;
  const int U = s.U, B = s.B, Kmax = s.Kmax, L = s.L, S = s.S;
  const bool use_graph = !(flags & UIS_FLAG_PROFILE) && (flags & UIS_FLAG_GRAPH);
  const bool per_step = (flags & UIS_FLAG_STEPWISE) != 0, generic = (flags & UIS_FLAG_GENERIC_SELECT) != 0;
  // (after a failed placement check the handle keeps to the launch-per-step path, unless UIS_FLAG_RESIDENT asks)
  const bool allowed = !resident_off || (flags & UIS_FLAG_RESIDENT);
  const long rows_per_utt = L == 1 ? (long)B : (long)s.NC;
  // (+ 16 rows of slack at look_ahead 1: room that a since removed kernel cut into two cohorts.  Kept: every buffer behind
  // `rows` in the workspace arena would move, and placement alone has measured a 4 % mode switch -- DESIGN.md section 5)
  static_cast<ClusterGeometry&>(p) = cluster_geometry(n_cu, U, rows_per_utt, L == 1 ? 16 : 0, s.G);
  p.max_rows = (long)U * rows_per_utt;
  p.hst = m.depth >= 2 && s.G == 1 &&
          ((m.Hp == 512 && (m.Dp == 128 || m.Dp == 256 || m.Dp == 512)) ||
           (m.Hp == 256 && (m.Dp == 128 || m.Dp == 256)) || (m.Hp == 128 && (m.Dp == 128 || m.Dp == 256)));
  // (the compile-time shape classes: unpadded models, and the embedded hidden sizes 257 .. 384, whose H_units is Hp)
  const bool exact = m.D == m.Dp && m.H_units == m.Hp;
  const bool c1 = exact && m.Hp == 512 && m.Dp == 256 && B == 10 && Kmax == 16;
  const bool c4 = exact && m.Hp == 512 && m.Dp == 512 && B == 20 && Kmax == 11;
  // (a model of the cluster kernels' shapes -- hidden size 128 with a small observation dim also counts as "small" --
  // goes to them: k_decode_big<WIN>)
  const bool cluster_shape = m.depth == 1 && (m.Hp == 128 || m.Hp == 256 || m.Hp == 512) && (m.Dp == 128 || m.Dp == 256 || m.Dp == 512);

  // the whole decode in one launch with register-resident weights (k_decode_resident and its relatives below); the
  // default wherever it applies.  (Its state is addressed through 2 GB buffer descriptors.)
  const bool resident_ok = L == 1 && s.G == 1 && !generic && resident_fits(m, U, B, Kmax, S, p);
  const bool resident = resident_ok && !use_graph && allowed && !per_step;
  // SMALL models (small_model_ok: hidden size up to about 64, any rnn_depth -- the shapes of the reference's own tests):
  // the whole beam search of an utterance on ONE workgroup (k_decode_small); look_ahead >= 2 with a sub-step of the
  // window kernel in the select's place
  const bool small_shape = s.G == 1 && !use_graph && !per_step && !generic && small_model_ok(m.Hp, m.Dp, m.depth);
  // rnn_depth >= 2 at the cluster kernels' shapes: k_decode_big's stages with the weight slot refilled per stage
  // (look_ahead >= 2: with the window's sub-step as the select stage, for the shapes instantiated)
  const bool deep_win_shape = (m.Hp == 512 && m.Dp == 256) || (m.Hp == 256 && (m.Dp == 128 || m.Dp == 256)) || (m.Hp == 128 && m.Dp == 128);
  const bool deep = p.hst && !small_shape && !use_graph && p.ncl >= 1 &&
                    (L == 1 ? select_fast_ok(B, Kmax, S) : deep_win_shape && big_win_lds_bytes(m.Hp, S, (int)s.NC, Kmax, B) <= 157 * 1024) &&
                    !per_step && !generic && allowed &&
                    ((double)U * S + 1) * m.depth * m.Hp * 4.0 < 2.0e9 && (double)p.rows_cap * m.G * 4.0 < 2.0e9 &&
                    (double)U * S * m.Dp * 4.0 < 2.0e9 && (L > 1 || deep_lds_bytes(m.Hp, m.Dp, B, Kmax, S) <= 157 * 1024);
  const bool small = !resident_ok && small_shape &&
                     (L == 1 ? select_fast_ok(B, Kmax, S) && small_lds_bytes(m.Dp, B, Kmax, S) <= 160 * 1024
                             : !cluster_shape && s.window_scratch <= 128 * 1024 && (double)U * s.NC * std::max(m.G, m.Hp) * 4.0 < 2.0e9);
  // look_ahead >= 2 in one launch (k_decode_big<WIN>: the window kernel's sub-step as the select stage of the
  // wave-per-row-tile decode; its state through 4 GB descriptors with unsigned offsets, element counts below 2^31)
  const bool win = !small && L > 1 && cluster_shape && s.G == 1 && !use_graph && p.ncl >= 1 && !per_step && allowed &&
                   ((double)U * S + 1) * m.Hp * 4.0 < 4.0e9 && (double)p.rows_cap * m.Hp * 4.0 < 4.0e9 &&
                   ((double)U * S + 1) * m.Hp < 2.0e9 && (double)U * S * m.Dp * 4.0 < 4.0e9 &&
                   big_win_lds_bytes(m.Hp, S, (int)s.NC, Kmax, B) <= 157 * 1024;

  if (resident) {
    const bool owner = (flags & UIS_FLAG_OWNER_SELECT) != 0 || s.biased || s.hinted || s.turned;
    const int per_xcd = (U + p.ncl - 1) / p.ncl;
    // (k_decode_rs keeps frame numbers in 32 bits and reads the frame stream through 4 GB descriptors with 32-bit byte
    // offsets: a row of gi0 is 3 Hp floats, a row of x Dp)
    const bool frames32 = s.F < 0x7fffffffLL && (double)s.F * std::max(3 * m.Hp, m.Dp) * 4.0 < 4.0e9;
    // (... and everything else its step loop addresses through ONE descriptor over the workspace from pool_mean to mse_tab
    // -- RsArgs, uis_kernels.h.  place_workspace sums that stretch from the workspace list itself and plan_and_place plans
    // again with k.no_rs set should it ever pass 4 GB: the next kernel then decodes, as for any other term below)
    const bool rs_block = !k.no_rs;
    // the REPLICATED select (k_decode_rs, uis_select_rs.hip): every workgroup of an XCD decides all of the cluster's
    // utterances, one wave each; the default where it applies (UIS_FLAG_OWNER_SELECT keeps k_decode_resident)
    if (!owner && m.Dp <= 256 && rs_select_ok(B, Kmax, S, (long)s.maxT) && frames32 && rs_block && per_xcd <= UIS_RS_UTT &&
        resident_rs_lds_bytes(m.Hp, m.Dp, B, Kmax, S) <= 160 * 1024)
      p.rs_kind = c1 ? RS_C1 : RS_BASE;
    // more utterances than workgroups: k_decode_big, whose dense stages give a wave a whole row tile (+6 % at 288
    // utterances, +17 % at 768 / 1024; UIS_FLAG_SMALL_TILES keeps the split-K passes: A/B switch, bit-identical) --
    // with the selects of a rank's utterances running concurrently, one wave each (k_decode_big<WS>), where the
    // single-wave select applies.  It takes over (round 5, profiles/r05_usweep_dispatch.json: 128 utterances 2.03
    // against 1.89 M frames/s, 160: 2.20 / 2.22, 192: 2.31 / 2.46, 224: 2.42 / 2.52, 256: 2.43 / 2.65) from 21
    // utterances per XCD with the concurrent selects, from 33 without them (profiles/r05_usweep_c4_shape.json: a tie at 128)
    const int per_rank = ((U + p.nclq - 1) / p.nclq + 31) / 32;
    const bool ws_shape = !owner && m.Dp <= 256 && per_rank <= 8 && rs_select_ok(B, Kmax, S, (long)s.maxT) &&
                          big_ws_lds_bytes(m.Hp, m.Dp, B, Kmax, S, per_rank) <= 160 * 1024;
    const bool big = U >= (ws_shape ? 20 : 32) * p.ncl + 1 && !(flags & UIS_FLAG_SMALL_TILES) &&
                     big_lds_bytes(m.Hp, m.Dp, B, Kmax, S) <= 160 * 1024;
    if (p.rs_kind != RS_NONE) {
      p.path = DecodePath::RS;
      p.cls = p.rs_kind == RS_C1 ? CLS_C1 : CLS_NONE;
      p.lds = resident_rs_lds_bytes(m.Hp, m.Dp, B, Kmax, S);
      p.decode_kernel = UIS_DK_RS | (p.rs_kind << 16);
    } else if (big && ws_shape) {
      p.path = DecodePath::BIG_WS;
      p.cls = c1 ? CLS_C1 : CLS_NONE;
      p.lds = big_ws_lds_bytes(m.Hp, m.Dp, B, Kmax, S, per_rank);
      p.decode_kernel = UIS_DK_BIG_WS;
    } else if (big) {
      p.path = DecodePath::BIG;
      p.lds = big_lds_bytes(m.Hp, m.Dp, B, Kmax, S);
      p.decode_kernel = UIS_DK_BIG;
    } else {
      p.path = DecodePath::RESIDENT;
      p.cls = c1 ? CLS_C1 : c4 ? CLS_C4 : CLS_NONE;
      p.lds = resident_lds_bytes(m.Hp, m.Dp, B, Kmax, S);
      p.decode_kernel = UIS_DK_RESIDENT;
    }
    p.lds = one_launch_lds(p.lds);
  } else if (win) {
    p.path = DecodePath::WINDOW;
    p.cls = exact && m.Hp == 512 && m.Dp == 256 && B == 50 && Kmax == 12 && L == 2 && s.NC == (int64_t)B * (Kmax + 1) &&
                    S == B * Kmax + B + B * (Kmax + 1) ? CLS_C2 : CLS_NONE;
    p.lds = big_win_lds_bytes(m.Hp, S, (int)s.NC, Kmax, B);
    p.decode_kernel = UIS_DK_WINDOW;
  } else if (deep) {
    p.path = DecodePath::DEEP;
    p.lds = L == 1 ? deep_lds_bytes(m.Hp, m.Dp, B, Kmax, S) : big_win_lds_bytes(m.Hp, S, (int)s.NC, Kmax, B);
    p.decode_kernel = UIS_DK_DEEP;
  } else if (small) {
    p.path = DecodePath::SMALL;
    p.lds = L == 1 ? small_lds_bytes(m.Dp, B, Kmax, S) : small_win_lds_bytes(S, (int)s.NC, Kmax, B);
    p.decode_kernel = UIS_DK_SMALL;
  } else {
    p.path = use_graph ? DecodePath::GRAPH : DecodePath::STEPWISE;
    p.lds = s.select_lds;
    p.decode_kernel = UIS_DK_STEPWISE | (dense_family(m, n_cu, flags, (long)(U / s.G) * (L == 1 ? B : (long)s.NC)) << 8);
  }

  // ---- (round 5) ingestion overlapped with the decode.  The one-launch kernels own every CU, so nothing can be
  // copied-and-projected "behind" them -- but k_decode_rs / k_decode_big<WS> / k_decode_resident (one utterance per
  // workgroup) can stop after any step and pick up again (DecodeState::step0 / step1 / resume).  For a list of
  // equal-length utterances given in HOST memory the decode is several launches: the first slice of every utterance's
  // frames travels (one strided copy) and is projected, the first launch decodes the steps that need nothing else (a
  // step looks one frame ahead: the early MSEs and the partial sums of the next select), the next slice travels and is
  // projected behind it, and so on.  What is left exposed of the PCIe leg is the first slice.
  // (utterances of equal length: a slice is ONE strided copy and the projection's batches are a constant stride apart.
  // A ragged list: only through the float64 entry, whose staging block the library lays out itself -- slice after
  // slice, so that a slice is one copy too, scattered to the utterance-major frame stream on the device; a copy per
  // utterance and slice measured 2.48 against 3.59 M frames/s at a ragged configs[3] share -- and from 64 MB of frames
  // on: a ragged configs[1] (24 MB) loses 3-5 % to the extra launches, 256 ragged utterances (96 MB) gain 2 %)
  // (... and a list too small to spend a launch on keeps one: below 8 MB of frames the whole copy takes less than the
  // ~0.15 ms a further launch costs)
  const double split_min_bytes = k.split_min_set ? k.split_min_bytes : (s.ragged ? 64e6 : 8e6);
  const bool big_enough = (double)s.F * m.D * 4.0 >= split_min_bytes;
  p.stage = s.f64 && s.host_frames && s.F > 0 && s.ragged && big_enough;
  const bool can_split = (!s.ragged || s.f64) && big_enough && s.host_frames && s.F > 0 &&
                         (p.path == DecodePath::RS || p.path == DecodePath::BIG_WS || (p.path == DecodePath::RESIDENT && U <= 32 * p.nclq)) &&
                         !(flags & (UIS_FLAG_PROFILE | UIS_FLAG_DEBUG_SCORES | UIS_FLAG_SMALL_TILES)) && m.D == m.Dp && !k.no_split;
  const int64_t uniN = s.maxN;  // the longest utterance: slice boundaries are frame indices inside an utterance
  if (can_split && uniN >= 128) {
    std::vector<int64_t>& cuts = p.cuts;
    if (k.split_frames_set) {
      for (long v : k.split_frames) {
        const int64_t lo = cuts.empty() ? 32 : cuts.back() + 32;
        if (lo <= uniN - 32 && cuts.size() < 7) cuts.push_back(std::max<int64_t>(lo, std::min<int64_t>(v, uniN - 32)));
      }
    } else {
      // A launch must last as long as the next slice travels, and every further launch costs ~0.15 ms (measured:
      // configs[1] with cuts 32 | 32,128 | 32,96,288: 1.622 / 1.604 / 1.591 M frames/s from pinned float32).  Model:
      // a decode step takes ~(11.7 + 0.108 U) us (profiles/r05_usweep.json), a frame of every utterance U D 4 bytes at
      // ~45 GB/s (a quarter more through the float64 cast); slice k + 1 = what travels during 0.9 of launch k, and a
      // last slice below a quarter of the utterance is not worth a launch of its own.
      const double step_us = 11.7 + 0.108 * U, frame_us = (double)U * m.D * 4.0 / 45e3 * (s.f64 ? 1.25 : 1.0);
      // (round 6) ... and no further cut once everything that is left travels within the launch in front of it plus two
      // relaunches' worth (0.3 ms): configs[1] got the cuts {32, 326} and paid a second relaunch for frames that had
      // arrived five milliseconds earlier -- 1.607 M frames/s through the float64 list against 1.629 M with the one cut
      // at 32 (profiles/r06_f64_leg_knobs.txt); the configs[3] share keeps its slices (a launch there lasts 4 ms, the rest 28)
      int64_t prev = 0, cur = 32;
      while (cur <= uniN - 32 && (int)cuts.size() < 6) {
        if (!cuts.empty() && uniN - cur < uniN / 4) break;
        cuts.push_back(cur);
        if ((double)(uniN - cur) * frame_us <= (double)(cur - prev) * step_us + 300.0) break;
        const int64_t next = cur + std::max<int64_t>(32, (int64_t)(0.9 * (double)(cur - prev) * step_us / frame_us));
        prev = cur; cur = next;
      }
    }
  }
  p.split = !p.cuts.empty();
  return p;
}

typedef void (*DecodeKernel)(DevModel, DecodeState);
typedef void (*RsKernel)(RsArgs);  // k_decode_rs takes its own compact argument block (uis_kernels.h)
template <typename Fn> struct KernelEntryOf { int Hp, Dp, variant; Fn fn; };
typedef KernelEntryOf<DecodeKernel> KernelEntry;

void kernel_table_tag(const void* table, KernelPick* pick);  // (below the tables)

// `pick`: the entry found, as the table itself states it (left alone where there is none).
template <typename Fn, size_t N>
Fn find_kernel(const KernelEntryOf<Fn> (&table)[N], int Hp, int Dp, int variant, KernelPick* pick = nullptr) {
  for (const KernelEntryOf<Fn>& e : table)
    if (e.Hp == Hp && e.Dp == Dp && e.variant == variant) {
      if (pick) {
        kernel_table_tag(table, pick);
        pick->Hp = e.Hp; pick->Dp = e.Dp; pick->variant = e.variant;
      }
      return e.fn;
    }
  return nullptr;
}

// The instantiations of the cluster-wide one-launch kernels, family by family (persist: a UIS_FLAG_PERSISTENT session's
// launch), keyed by (Hp, Dp, variant): variant = the shape class (CLS_*), for k_decode_rs its kind (RS_*), for
// k_decode_deep look_ahead >= 2.
namespace kernels {
const KernelEntry big_ws[] = {
    {512, 256, CLS_C1, &k_decode_big<512, 256, true, 10, 16>},
    {512, 256, CLS_NONE, &k_decode_big<512, 256, true>}, {512, 128, CLS_NONE, &k_decode_big<512, 128, true>},
    {256, 256, CLS_NONE, &k_decode_big<256, 256, true>}, {256, 128, CLS_NONE, &k_decode_big<256, 128, true>},
    {128, 256, CLS_NONE, &k_decode_big<128, 256, true>}, {128, 128, CLS_NONE, &k_decode_big<128, 128, true>}};
const KernelEntryOf<RsKernel> rs[] = {
    {512, 256, RS_BASE, &k_decode_rs<512, 256>}, {512, 128, RS_BASE, &k_decode_rs<512, 128>},
    {256, 256, RS_BASE, &k_decode_rs<256, 256>}, {256, 128, RS_BASE, &k_decode_rs<256, 128>},
    {128, 256, RS_BASE, &k_decode_rs<128, 256>}, {128, 128, RS_BASE, &k_decode_rs<128, 128>},
    {512, 256, RS_C1, &k_decode_rs<512, 256, 10, 16>}};
// the same entries for a decode with limits (uis_decode_limits): not a table of its own to the outside -- a decode reports
// the entry of `rs` it stands for
const KernelEntryOf<RsKernel> rs_lim[] = {
    {512, 256, RS_BASE, &k_decode_rs<512, 256, 0, -1>}, {512, 128, RS_BASE, &k_decode_rs<512, 128, 0, -1>},
    {256, 256, RS_BASE, &k_decode_rs<256, 256, 0, -1>}, {256, 128, RS_BASE, &k_decode_rs<256, 128, 0, -1>},
    {128, 256, RS_BASE, &k_decode_rs<128, 256, 0, -1>}, {128, 128, RS_BASE, &k_decode_rs<128, 128, 0, -1>},
    {512, 256, RS_C1, &k_decode_rs<512, 256, 10, -16>}};
const KernelEntry resident[] = {
    {512, 256, CLS_C1, &k_decode_resident<512, 256, false, 10, 16>}, {512, 512, CLS_C4, &k_decode_resident<512, 512, false, 20, 11>},
    {512, 256, CLS_NONE, &k_decode_resident<512, 256>}, {512, 512, CLS_NONE, &k_decode_resident<512, 512>},
    {512, 128, CLS_NONE, &k_decode_resident<512, 128>}, {256, 256, CLS_NONE, &k_decode_resident<256, 256>},
    {256, 128, CLS_NONE, &k_decode_resident<256, 128>}, {256, 512, CLS_NONE, &k_decode_resident<256, 512>},
    {128, 256, CLS_NONE, &k_decode_resident<128, 256>}, {128, 128, CLS_NONE, &k_decode_resident<128, 128>},
    {128, 512, CLS_NONE, &k_decode_resident<128, 512>}};
const KernelEntry big[] = {
    {512, 256, CLS_NONE, &k_decode_big<512, 256>}, {512, 512, CLS_NONE, &k_decode_big<512, 512>},
    {512, 128, CLS_NONE, &k_decode_big<512, 128>}, {256, 256, CLS_NONE, &k_decode_big<256, 256>},
    {256, 128, CLS_NONE, &k_decode_big<256, 128>}, {256, 512, CLS_NONE, &k_decode_big<256, 512>},
    {128, 256, CLS_NONE, &k_decode_big<128, 256>}, {128, 128, CLS_NONE, &k_decode_big<128, 128>},
    {128, 512, CLS_NONE, &k_decode_big<128, 512>}};
const KernelEntry window[] = {
    {512, 256, CLS_C2, &k_decode_big<512, 256, false, 50, 12, true>},
    {512, 256, CLS_NONE, &k_decode_big<512, 256, false, 0, 0, true>}, {512, 128, CLS_NONE, &k_decode_big<512, 128, false, 0, 0, true>},
    {512, 512, CLS_NONE, &k_decode_big<512, 512, false, 0, 0, true>}, {256, 256, CLS_NONE, &k_decode_big<256, 256, false, 0, 0, true>},
    {256, 128, CLS_NONE, &k_decode_big<256, 128, false, 0, 0, true>}, {256, 512, CLS_NONE, &k_decode_big<256, 512, false, 0, 0, true>},
    {128, 256, CLS_NONE, &k_decode_big<128, 256, false, 0, 0, true>}, {128, 128, CLS_NONE, &k_decode_big<128, 128, false, 0, 0, true>},
    {128, 512, CLS_NONE, &k_decode_big<128, 512, false, 0, 0, true>}};
const KernelEntry deep[] = {
    {512, 256, 0, &k_decode_deep<512, 256>}, {512, 128, 0, &k_decode_deep<512, 128>}, {512, 512, 0, &k_decode_deep<512, 512>},
    {256, 256, 0, &k_decode_deep<256, 256>}, {256, 128, 0, &k_decode_deep<256, 128>}, {128, 128, 0, &k_decode_deep<128, 128>},
    {128, 256, 0, &k_decode_deep<128, 256>},
    {512, 256, 1, &k_decode_deep<512, 256, true>}, {256, 256, 1, &k_decode_deep<256, 256, true>},
    {256, 128, 1, &k_decode_deep<256, 128, true>}, {128, 128, 1, &k_decode_deep<128, 128, true>}};
const KernelEntry persist[] = {
    {512, 256, CLS_NONE, &k_decode_resident<512, 256, true>}, {512, 512, CLS_NONE, &k_decode_resident<512, 512, true>},
    {256, 256, CLS_NONE, &k_decode_resident<256, 256, true>}};
}  // namespace kernels

// Every table with the family it reports (UIS_DK_*) and whether it is the persist table: the one list behind a lookup's
// record (kernel_table_tag) and uis_decode_kernel_table.
template <typename F>
void for_each_kernel_table(F&& f) {
  f(kernels::rs, UIS_DK_RS, 0); f(kernels::resident, UIS_DK_RESIDENT, 0); f(kernels::big, UIS_DK_BIG, 0);
  f(kernels::big_ws, UIS_DK_BIG_WS, 0); f(kernels::window, UIS_DK_WINDOW, 0); f(kernels::deep, UIS_DK_DEEP, 0);
  f(kernels::persist, UIS_DK_RESIDENT, 1);
}

void kernel_table_tag(const void* table, KernelPick* pick) {
  for_each_kernel_table([&](const auto& t, int family, int persist) {
    if (static_cast<const void*>(t) == table) { pick->family = family; pick->persist = persist; }
  });
}

DecodeKernel cluster_kernel(const DecodePlan& p, const DevModel& m, int L, KernelPick* pick) {
  switch (p.path) {
    case DecodePath::BIG_WS: return find_kernel(kernels::big_ws, m.Hp, m.Dp, p.cls, pick);
    case DecodePath::RESIDENT: return find_kernel(kernels::resident, m.Hp, m.Dp, p.cls, pick);
    case DecodePath::BIG: return find_kernel(kernels::big, m.Hp, m.Dp, p.cls, pick);
    case DecodePath::WINDOW: return find_kernel(kernels::window, m.Hp, m.Dp, p.cls, pick);
    case DecodePath::DEEP: return find_kernel(kernels::deep, m.Hp, m.Dp, L > 1 ? 1 : 0, pick);
    default: return nullptr;
  }
}

// One launch of a cluster-wide decode kernel: a workgroup of 512 threads on every CU of the ncl clusters.
int launch_cluster_kernel(Launcher& lch, DecodeKernel kern, int n_cu, int ncl, size_t lds, const DevModel& m, const DecodeState& st,
                          bool cooperative = true) {
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return lch.run_cooperative(UIS_K_GRU, kern, n_cu, dim3(32 * ncl), dim3(512), lds, cooperative, m, st);
}

// k_decode_rs's argument block from the decode's model and state.  Everything its step loop addresses in the workspace
// -- the pools, the row tiles, the MSE tables, the control words, what it leaves for k_backtrace -- is named by a 32-bit
// offset from pool_mean, the first of them in the arena (plan_decode keeps that stretch below 4 GB; checked again here).
int rs_make_args(const DevModel& m, const DecodeState& st, size_t bp_bytes, RsArgs* out) {
  RsArgs a{};
  a.U = st.U; a.B = st.B; a.Kmax = st.Kmax; a.S = st.S; a.D = m.D; a.H_units = m.H_units; a.tau = st.tau;
  a.ncl = st.ncl; a.rx_stride = st.rx_stride; a.step0 = st.step0; a.step1 = st.step1; a.flags = st.flags;
  a.lp_stay = m.lp_stay; a.lp_sw = m.lp_sw; a.lp_new = m.lp_new;
  a.whh = m.whh[0]; a.w1 = m.w1; a.w2 = m.w2; a.bhh = m.bhh[0]; a.b1 = m.b1; a.b2 = m.b2; a.wgt = m.wgt;
  a.off = st.off; a.resume = st.resume; a.limit = st.limit;
  a.logblk = st.logblk; a.logden = st.logden;
  a.x = st.x; a.gi0 = st.gi0; a.mse0 = st.mse0;
  a.overflow = st.overflow; a.dbg_scores = st.dbg_scores; a.counters = st.counters;
  // (the kernel tests the bit every step and reads the pointer behind it only)
  a.flags = st.dbg_scores ? a.flags | UIS_FLAG_DEBUG_SCORES : a.flags & ~UIS_FLAG_DEBUG_SCORES;
  a.blk = reinterpret_cast<unsigned char*>(st.pool_mean);
  bool ok = true;
  auto at = [&](const void* p, size_t bytes) -> uint32_t {
    const unsigned char* q = static_cast<const unsigned char*>(p);
    if (q < a.blk || (size_t)(q - a.blk) + bytes >= ((size_t)1 << 32)) { ok = false; return 0u; }
    return (uint32_t)(q - a.blk);
  };
  const size_t rows = (size_t)st.ncl * st.rx_stride, US = (size_t)st.U * st.S;
  a.o_mean = at(st.pool_mean, US * m.Dp * 4);
  a.o_hid = at(st.pool_hid, (US + 1) * m.Hp * 4);
  a.o_h1 = a.o_hid + (uint32_t)(US * m.Hp * 4);
  a.o_hst = at(st.gi_up, rows * m.Hp * 4);
  a.o_a1 = at(st.a1, rows * m.Hp * 4);
  a.o_tab = at(st.mse_tab, 2 * US * 4);
  a.o_part = at(st.mse_part, rows * rs_part_stride(m.Dp) * 4);
  a.o_ctl = at(st.cl_xcc, 0);
  a.o_flag_word = (uint32_t)(st.rx_flags - st.cl_xcc);
  ok = ok && st.cl_abort == st.cl_xcc + 16 && st.rx_flags > st.cl_xcc;
  (void)at(st.rx_flags, (size_t)st.ncl * 128);
  a.o_beam_n = at(st.beam_n, (size_t)2 * st.U * 4);
  a.o_beam_score = at(st.beam_score, (size_t)2 * st.U * st.B * 4);
  a.o_bp = at(st.bp, bp_bytes);
  if (!ok) return fail(UIS_ERR_HIP, "k_decode_rs: its workspace is not one stretch below 4 GB");
  *out = a;
  return UIS_OK;
}

int launch_rs_kernel(Launcher& lch, RsKernel kern, int n_cu, int ncl, size_t lds, const DevModel& m, const DecodeState& st, size_t bp_bytes) {
  RsArgs a;
  if (int rc = rs_make_args(m, st, bp_bytes, &a)) return rc;
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return lch.run_cooperative(UIS_K_GRU, kern, n_cu, dim3(32 * ncl), dim3(512), lds, true, a);
}

#if defined(UIS_SELECT_TIMING) || defined(UIS_RESIDENT_PROBE) || defined(UIS_RS_COUNT_PATHS) || defined(UIS_RESIDENT_TIMING)
// Diagnostic builds: what the device-side counters of the decode just run recorded, on stderr.
int report_diagnostics(uis_handle* h, const DecodePlan& plan, int U, int64_t maxT, int L) {
#if defined(UIS_SELECT_TIMING)
  {
    unsigned long long tc[48];
    HIPCHK(hipMemcpy(tc, h->counters.as<unsigned long long>(), sizeof(tc), hipMemcpyDeviceToHost));
    const double launches = (double)maxT * U;
    if (L == 1) {
      fprintf(stderr, "[select timing] cycles per workgroup-launch:");
      for (int k = 0; k < 8; ++k) fprintf(stderr, " p%d=%.0f", k, (double)tc[16 + k] / launches);
      fprintf(stderr, "\n");
    } else {
      static const char* names[7] = {"live+offsets", "mse", "scores", "expand/prune", "leaders+slots", "tables", "records+rows"};
      for (int half = 0; half < 2; ++half) {
        const unsigned long long* c = tc + (half ? 32 : 16);
        const double n = (double)std::max<unsigned long long>(c[7], 1);
        fprintf(stderr, "[window timing] %s sub-steps, us per workgroup-launch:", half ? "pruning" : "expanding");
        double sum = 0.0;
        for (int k = 0; k < 7; ++k) { fprintf(stderr, " %s=%.2f", names[k], (double)c[k] * 0.01 / n); sum += (double)c[k] * 0.01 / n; }
        fprintf(stderr, " | total=%.2f; per launch: candidates=%.0f live=%.0f hypotheses in=%.0f rows=%.1f\n", sum, (double)c[8] / n,
                (double)c[9] / n, (double)c[10] / n, (double)c[11] / n);
      }
    }
  }
#endif
#if defined(UIS_RESIDENT_PROBE)
  if (plan.resident()) {
    unsigned long long tc[88];
    HIPCHK(hipMemcpy(tc, h->counters.as<unsigned long long>(), sizeof(tc), hipMemcpyDeviceToHost));
    fprintf(stderr, "[resident probe] cycles per dependent load: own-table(nt)=%.0f mean(sc1)=%.0f wgt(plain)=%.0f wgt-again=%.0f\n",
            (double)tc[80] / (double)maxT, (double)tc[81] / (double)maxT, (double)tc[82] / (double)maxT, (double)tc[83] / (double)maxT);
  }
#endif
#if defined(UIS_RS_COUNT_PATHS)
  if (plan.path == DecodePath::RS) {
    unsigned long long tc[96];
    HIPCHK(hipMemcpy(tc, h->counters.as<unsigned long long>(), sizeof(tc), hipMemcpyDeviceToHost));
    fprintf(stderr, "[rs short lists] selects with <= 16 / <= 32 / <= 64 / more survivors: %llu %llu %llu %llu\n", tc[88], tc[89], tc[90], tc[91]);
  }
#endif
#if defined(UIS_RESIDENT_TIMING)
  if (plan.path == DecodePath::WINDOW) {  // even sub-steps (expanding, at look_ahead 2) and odd ones (pruning) apart
    const int ncl = plan.ncl;
    unsigned long long tc[88];
    HIPCHK(hipMemcpy(tc, h->counters.as<unsigned long long>(), sizeof(tc), hipMemcpyDeviceToHost));
    static const char* names[8] = {"window", "barA", "gru", "barB", "head1", "barC", "head2", "barD"};
    for (int wg = 0; wg < 2; ++wg)
      for (int odd = 0; odd < 2; ++odd) {
        fprintf(stderr, "[window launch timing] workgroup %3d, %s sub-steps, us per sub-step:", wg ? 248 : 0, odd ? "odd" : "even");
        double sum = 0.0;
        for (int k = 0; k < 8; ++k) {
          const double us = (double)tc[(wg ? 64 : 48) + 8 * odd + k] * 0.01 / ((double)maxT * 0.5);
          fprintf(stderr, " %s=%.2f", names[k], us);
          sum += us;
        }
        fprintf(stderr, " | total=%.2f\n", sum);
      }
    std::vector<unsigned long long> per((size_t)96 + 1024);
    HIPCHK(hipMemcpy(per.data(), h->counters.as<unsigned long long>(), per.size() * 8, hipMemcpyDeviceToHost));
    for (int wg = 0; wg < 2; ++wg) {
      fprintf(stderr, "[window launch timing] workgroup %3d, gru of the even sub-steps, us by wave:", wg ? 248 : 0);
      for (int w = 0; w < 8; ++w) fprintf(stderr, " %.1f", (double)per[80 + 8 * wg + w] * 0.01 / ((double)maxT * 0.5));
      fprintf(stderr, "\n");
    }
    static const char* what[4] = {"gru", "wait B", "head1", "head2"};
    for (int k = 0; k < 4; ++k) {
      fprintf(stderr, "[window launch timing] %s, even sub-steps, us by rank (mean over the clusters):", what[k]);
      for (int r = 0; r < 32; ++r) {
        double sum = 0.0;
        for (int c = 0; c < ncl; ++c) sum += (double)per[(size_t)96 + 256 * k + c + ncl * r];
        fprintf(stderr, " %.1f", sum / ncl * 0.01 / ((double)maxT * 0.5));
      }
      fprintf(stderr, "\n");
    }
  }
  if (plan.resident()) {
    unsigned long long tc[88];
    HIPCHK(hipMemcpy(tc, h->counters.as<unsigned long long>(), sizeof(tc), hipMemcpyDeviceToHost));
    static const char* names[8] = {"select", "barA", "gru", "barB", "head1", "barC", "head2", "barD"};
    for (int wg = 0; wg < 2; ++wg) {
      fprintf(stderr, "[resident timing] workgroup %3d, us per step:", wg ? 248 : 0);
      for (int k = 0; k < 8; ++k) fprintf(stderr, " %s=%.2f", names[k], (double)tc[(wg ? 64 : 48) + k] * 0.01 / (double)maxT);
      fprintf(stderr, "\n");
    }
    fprintf(stderr, "[resident timing] select phases (wg 0), us per step:");
    for (int k = 0; k < 8; ++k) fprintf(stderr, " p%d=%.2f", k, (double)tc[80 + k] * 0.01 / (double)maxT);
    fprintf(stderr, "\n");
    fprintf(stderr, "[resident timing] gru fine (wg 248): other=%.2f tile=%.2f combine=%.2f sync=%.2f\n",
            (double)tc[72] * 0.01 / (double)maxT, (double)tc[73] * 0.01 / (double)maxT, (double)tc[74] * 0.01 / (double)maxT,
            (double)tc[75] * 0.01 / (double)maxT);
    if (plan.path == DecodePath::BIG || plan.path == DecodePath::BIG_WS) {  // k_decode_big: the GRU stage wave by wave, the row tiles per step
      unsigned long long wv[32];
      HIPCHK(hipMemcpy(wv, h->counters.as<unsigned long long>() + 96, sizeof(wv), hipMemcpyDeviceToHost));
      for (int wg = 0; wg < 2; ++wg) {
        fprintf(stderr, "[resident timing] workgroup %3d, gru us per step by wave:", wg ? 248 : 0);
        for (int w = 0; w < 8; ++w) fprintf(stderr, " %.1f", (double)wv[8 * wg + w] * 0.01 / (double)maxT);
        fprintf(stderr, "\n");
      }
      fprintf(stderr, "[resident timing] cluster 0: row tiles per step mean %.2f; steps by (row tiles mod 8):", (double)wv[24] / (double)maxT);
      for (int k = 0; k < 8; ++k) fprintf(stderr, " %d:%llu", k, wv[16 + k]);
      fprintf(stderr, "\n");
    }
  }
#endif
  return UIS_OK;
}
#endif

// ---- decode_once(): one uis_decode* call as a sequence of steps.  What the steps hand to each other:
struct DecodeCall {
  // the call as it came in
  uis_handle* h; const float* d_frames; const int64_t* offsets; int32_t n_utt; const uis_decode_opts* opts;
  int32_t* d_labels; float* d_scores; uis_stats* stats; const float* h_frames;
  DecodeKnobs knobs;
  // derive_shape
  DecodeShape shape{};
  int tau = 1;
  bool profile = false, dbg = false;
  WindowScratch wsl{};
  std::vector<GroupPlan> groups;
  std::vector<int64_t> bp_base;  // back-pointer records per utterance (the window machinery's): windows x B
  // plan_and_place
  DecodePlan plan;
  bool rs = false;
  size_t dbg_floats = 0;
  int64_t n_log = 0;
  size_t mse_tab_bytes = 0, mse_part_bytes = 0;
  DecodeKernel cluster_kern = nullptr;
  RsKernel rs_kern = nullptr;
  // ctl_choose
  bool ctl_tune = false;
  uint32_t* ctl = nullptr;
  // upload_tables
  const float* d_x = nullptr;    // the frames as the kernels read them: padded where D is no multiple of 16
  std::vector<double> log_host;  // (the source of asynchronous copies: lives until the call's streams are drained)
};

}  // namespace

#include "uis_workspace.hip"

namespace {

// How many utterances hit the cluster cap (their flags to overflow_out, if given), and the status every entry point
// that reads labels returns for that count.
int count_cluster_cap(const std::vector<int32_t>& overflow, int32_t* overflow_out = nullptr) {
  int n_over = 0;
  for (size_t u = 0; u < overflow.size(); ++u) {
    if (overflow_out) overflow_out[u] = overflow[u];
    n_over += overflow[u] != 0;
  }
  return n_over;
}
int cluster_cap_status(int n_over, int Kmax) {
  if (!n_over) return UIS_OK;
  return fail(UIS_ERR_CLUSTER_CAP, std::to_string(n_over) + " utterance(s) needed more than max_clusters=" +
                                       std::to_string(Kmax) + " clusters per hypothesis");
}

// Whether the running call's uis_min_turn table sets a rule for any utterance (0 and 1 set none: such a decode is
// planned, laid out and run as one without a table).
static bool turn_rule(const uis_handle* h) {
  bool any = false;
  for (int32_t v : h->tables.min_turn.call) any = any || v >= 2;
  return h->tables.min_turn.call_set && any;
}

// Step 1: the arguments checked, the DecodeShape and the utterance groups.  shape.U == 0 with UIS_OK: an empty list,
// nothing left to do.
int derive_shape(DecodeCall& c) {
  uis_handle* h = c.h;
  const int64_t* offsets = c.offsets;
  const uis_decode_opts* opts = c.opts;
  const int32_t n_utt = c.n_utt;
  // (whatever refuses this decode below: uis_last_decode_info must not hand out the PREVIOUS decode's arrays)
  h->last_U = 0; h->last_B = 0;
  h->last_overflow.clear(); h->last_beam_scores.clear();
  h->nb_valid = false;  // (... nor uis_last_decode_nbest its hypotheses)
  if (h->stream_state.active) return fail(UIS_ERR_INVALID_ARG, "a streaming session is open on this handle (uis_stream_end first)");
  if (int rc = table_status(h->tables.check_limits("decode", n_utt))) return rc;
  if (int rc = table_status(h->tables.check_min_turn("decode", n_utt))) return rc;
  h->last_pick = KernelPick{};
  const DevModel& m = h->m;
  const int B = opts->beam_size, L = opts->look_ahead, tau = opts->test_iteration;
  int Kmax = opts->max_clusters > 0 ? opts->max_clusters : 16;
  // (round 5: no option value the reference takes is refused for its size any more -- a beam beyond the select
  // kernels' 256, a cluster cap beyond their LDS budget and any look_ahead go through the window machinery, a launch
  // per sub-step with the candidate lists in HBM; what is left are the widths of the window records' fields)
  if (B < 1 || B > 32767) return fail(UIS_ERR_UNSUPPORTED, "beam_size must be in [1, 32767]");
  if (L < 1 || tau < 1) return fail(UIS_ERR_INVALID_ARG, "look_ahead and test_iteration must be >= 1");
  if (L > UIS_MAX_LOOKAHEAD) return fail(UIS_ERR_UNSUPPORTED, "look_ahead must be <= 1024");
  if (Kmax > 4096) return fail(UIS_ERR_UNSUPPORTED, "max_clusters must be <= 4096");
  if (opts->level_cap < 0) return fail(UIS_ERR_INVALID_ARG, "level_cap must be >= 0");
  const int64_t level_cap = opts->level_cap > 0 ? std::min<int64_t>(opts->level_cap, UIS_LEVEL_CAP_MAX) : UIS_LEVEL_CAP;
  if (offsets[0] != 0) return fail(UIS_ERR_INVALID_ARG, "offsets[0] must be 0");
  int64_t maxN = 0;
  for (int u = 0; u < n_utt; ++u) {
    const int64_t n = offsets[u + 1] - offsets[u];
    if (n < 0) return fail(UIS_ERR_INVALID_ARG, "offsets must be non-decreasing");
    maxN = std::max(maxN, n);
  }
  const int64_t F = n_utt ? offsets[n_utt] : 0;
  if (int rc = table_status(h->tables.check_bias("decode", F))) return rc;
  if (int rc = table_status(h->tables.check_hint("decode", F))) return rc;
  bool ragged_list = false;  // (utterances of different lengths)
  for (int u = 1; u < n_utt; ++u) ragged_list = ragged_list || offsets[u + 1] - offsets[u] != offsets[1] - offsets[0];
  if (c.stats) memset(c.stats, 0, sizeof(*c.stats));
  h->last_U = n_utt; h->last_B = B;
  h->last_overflow.assign(n_utt, 0);
  h->last_beam_scores.assign((size_t)n_utt * B, INFINITY);
  if (n_utt == 0) {
    h->nb_groups.clear(); h->nb_offsets.assign(1, 0); h->nb_B = B; h->nb_wnd = false; h->nb_valid = true;
    return UIS_OK;
  }
  if (F > 0 && (!c.d_frames || !c.d_labels)) return fail(UIS_ERR_INVALID_ARG, "frames/labels_out is null");
  const int64_t maxT = (int64_t)tau * maxN;
  if (maxT > 0x7fffff00LL) return fail(UIS_ERR_UNSUPPORTED, "test_iteration * N too large");
  // (a cluster's tag shares its block-count word: the count keeps bits 0 .. 23)
  if (h->tables.hint.call_set && maxT >= UIS_TAGGED_FRAMES_END)
    return fail(UIS_ERR_UNSUPPORTED, "a decode with known speakers (uis_frame_speakers) needs test_iteration * N below 2^24");
  HIPCHK(hipSetDevice(h->device));

  const int U = n_utt;
  // look_ahead >= 2: capacity of an intermediate level = every assignment of the window's first
  // j frames, N_j = B * prod_{i=1..j} (Kmax + i), capped; the slot pool holds the beam's states,
  // every level's new ones and the winners'.
  int64_t NC = B, S64 = (int64_t)B * Kmax + B;
  if (L > 1) {
    int64_t nj = B;
    NC = 0;
    for (int j2 = 1; j2 < L; ++j2) {
      nj = std::min<int64_t>(nj * (Kmax + j2), level_cap);
      NC = std::max(NC, nj);
      S64 += nj;
    }
  }
  if (S64 > 0x3fffffff) return fail(UIS_ERR_UNSUPPORTED, "beam_size * max_clusters ^ look_ahead too large");
  const int S = (int)S64;
  c.profile = (opts->flags & UIS_FLAG_PROFILE) != 0;
  c.dbg = (opts->flags & UIS_FLAG_DEBUG_SCORES) != 0;
  c.tau = tau;
  h->prof.used = 0; h->prof.cls.clear();

  // wnd: the window machinery decodes -- look_ahead >= 2, and look_ahead 1 where the select kernels do not apply
  // (beam_size > 256, or tables beyond their LDS budget): k_window with a window of ONE frame is the prune
  // sub-step alone, its work arrays in LDS where they fit and in HBM where they do not
  SelectLds lds{};
  bool wnd = L > 1 || B > 256;
  if (!wnd) {
    lds = select_lds_layout(m.Dp, B, Kmax, S);
    if (lds.total > 160 * 1024) wnd = true;
  }
  // (a field-width limit that no smaller list cures is UNSUPPORTED -- the Python host halves a list on UIS_ERR_OOM, which
  // only helps the term that grows with the number of utterances)
  if (NC * (int64_t)(Kmax + 1) > 0x3fffffff)
    return fail(UIS_ERR_UNSUPPORTED, "level capacity * max_clusters beyond the kernels' 32-bit indices");
  if ((int64_t)U * std::max<int64_t>(NC, B) > 0x3fffffff)
    return fail(UIS_ERR_OOM, "utterances * level capacity beyond the kernels' 32-bit indices");
  c.wsl = window_scratch_layout(S, (int)NC, Kmax, B);
  {  // refuse configurations whose state would not fit the device instead of failing in hipMalloc
    const double bytes = (double)U * S * (m.Dp + (double)m.depth * m.Hp) * 4.0 +
                         (wnd ? (double)U * (c.wsl.total + 2.0 * NC * (Kmax * 8.0 + 32.0) + NC * (m.Hp + m.G) * 4.0) : 0.0);
    if (bytes > c.knobs.max_state_bytes)
      return fail(UIS_ERR_OOM, "decode state would need " + std::to_string((long long)(bytes / 1e9)) + " GB");
  }

  // ---- utterance groups: independent lock-step chains, one stream each.  Measured on
  // MI355X: the device overlaps at most ~2 of these small kernels, so more
  // groups mean more launches, not more throughput -- the default is one group.
  int G = opts->n_streams > 0 ? opts->n_streams : 1;
  if (c.profile || c.dbg) G = 1;
  G = std::max(1, std::min(std::min(G, UIS_MAX_GROUPS), U));
  while ((int)h->gstreams.size() < G) {
    hipStream_t sgrp;
    HIPCHK(hipStreamCreateWithFlags(&sgrp, hipStreamNonBlocking));
    h->gstreams.push_back(sgrp);
  }
  if (int rc = grow_events(h->gdone, (size_t)G)) return rc;
  if ((int)h->gcache.size() < G) h->gcache.resize(G);
  c.groups.assign(G, GroupPlan{});
  for (int g = 0; g < G; ++g) {
    GroupPlan& gp = c.groups[g];
    gp.u0 = (int)((int64_t)U * g / G);
    gp.U = (int)((int64_t)U * (g + 1) / G) - gp.u0;
    for (int u = gp.u0; u < gp.u0 + gp.U; ++u) gp.maxT = std::max<int64_t>(gp.maxT, (int64_t)tau * (offsets[u + 1] - offsets[u]));
  }
  c.bp_base.assign(U + 1, 0);
  if (wnd)
    for (int u = 0; u < U; ++u)
      c.bp_base[u + 1] = c.bp_base[u] + (((int64_t)tau * (offsets[u + 1] - offsets[u]) + L - 1) / L) * B;
  c.shape = DecodeShape{U, G, B, Kmax, L, S, F, maxN, maxT, NC, ragged_list, h->src64 != nullptr, c.h_frames != nullptr,
                        wnd, (size_t)lds.total, c.wsl.total, h->tables.bias3.call_set, h->tables.hint.call_set, turn_rule(h)};
  return UIS_OK;
}

// Step 2: which kernels decode this list, and its workspace placed.  Planned a second time, without k_decode_rs, should
// that kernel's stretch of the workspace pass 4 GB (place_workspace).
int plan_and_place(DecodeCall& c) {
  uis_handle* h = c.h;
  const DevModel& m = h->m;
  const DecodeShape& s = c.shape;
  DecodeKnobs plan_knobs = c.knobs;
  for (;;) {
    c.plan = plan_decode(m, s, c.opts->flags, plan_knobs, h->n_cu, h->resident_off);
    if ((c.opts->flags & UIS_FLAG_RESIDENT) && !c.plan.one_launch())
      return fail(UIS_ERR_UNSUPPORTED, "UIS_FLAG_RESIDENT needs (look_ahead 1:) one stream, beam_size * (max_clusters + 1) <= 256, no "
                                       "per-step path flag and either a small model (rnn_hidden_size up to about 64, any rnn_depth) "
                                       "or rnn_depth 1 with rnn_hidden_size 128, 256 or 512 (padded), observation_dim 128, "
                                       "256 or 512 (padded) and a device whose CU count is a multiple of 32");
    c.rs = c.plan.path == DecodePath::RS;
    // one array per window: [windows][U][B][Kmax + 1] ^ look_ahead
    double dbg_want = c.dbg ? (double)((s.maxT + s.L - 1) / s.L) * s.U * s.B : 0.0;
    for (int k = 0; k < s.L; ++k) dbg_want *= (double)(s.Kmax + 1);
    if (dbg_want > 1e9) return fail(UIS_ERR_UNSUPPORTED, "UIS_FLAG_DEBUG_SCORES: more than 1e9 candidate scores (a test hook for small decodes)");
    c.dbg_floats = (size_t)dbg_want;
    h->dbg_floats = 0;
    const int rc = place_workspace(h, c.knobs, c.rs, workspace_list(c));
    if (rc == UIS_OK) break;
    if (rc != WS_REPLAN) return rc;
    plan_knobs.no_rs = true;
  }
  KernelPick pick;
  pick.family = c.plan.decode_kernel & 0xff; pick.Hp = m.Hp; pick.Dp = m.Dp;  // (what stays without a table lookup)
  c.cluster_kern = c.plan.clustered() && !c.rs ? cluster_kernel(c.plan, m, s.L, &pick) : nullptr;
  c.rs_kern = c.rs ? find_kernel(kernels::rs, m.Hp, m.Dp, c.plan.rs_kind, &pick) : nullptr;
  if (c.rs_kern && h->tables.limits.call_set) c.rs_kern = find_kernel(kernels::rs_lim, m.Hp, m.Dp, c.plan.rs_kind);  // (the same entry's twin)
  h->last_pick = pick;
  return UIS_OK;
}

// Step 3: where this decode's control words sit inside cluster_ctl (uis_handle::CtlTune) -- ctl_choose before the
// decode, ctl_record after it with the device time the placement got.
void ctl_choose(DecodeCall& c) {
  uis_handle* h = c.h;
  const DecodeShape& s = c.shape;
  uis_handle::CtlTune& tn = h->ctl_tune;
  int ctl_cand = 0;
  // (not for k_decode_rs: its row descriptors and row counters live in LDS, only the barrier
  // counters are polled in memory, and what is left of the placement effect is 1 % --
  // profiles/r03_bimodal.txt -- against 5 % for the kernels that keep them in global memory)
  c.ctl_tune = c.plan.resident() && !c.rs && !c.knobs.no_ctl_tune;
  if (c.ctl_tune) {
    const uint64_t sig = ((uint64_t)s.U << 44) ^ ((uint64_t)s.F << 16) ^ ((uint64_t)s.maxT << 6) ^ ((uint64_t)s.B << 1) ^ ((uint64_t)s.Kmax << 54);
    if (tn.sig != sig) { tn = uis_handle::CtlTune{}; tn.sig = sig; }
    ctl_cand = (tn.phase >= 1 && tn.phase <= 4) ? tn.phase - 1 : tn.best;
  }
  size_t ctl_off = kCtlPlace[ctl_cand];
  if (c.knobs.ctl_offset_set) ctl_off = std::min<size_t>(c.knobs.ctl_offset, kCtlPlace[3]);  // experiments
  c.ctl = reinterpret_cast<uint32_t*>(h->cluster_ctl.as<char>() + ctl_off);
}

int ctl_record(DecodeCall& c) {
  uis_handle::CtlTune& tn = c.h->ctl_tune;
  if (!(c.ctl_tune && tn.sig != 0 && tn.phase <= 4)) return UIS_OK;
  float ms = 0.0f;
  HIPCHK(hipEventElapsedTime(&ms, c.h->ev_begin, c.h->ev_end));
  if (tn.phase >= 1) tn.ms[tn.phase - 1] = ms;
  if (++tn.phase == 5) {
    tn.best = 0;
    for (int k = 1; k < 4; ++k)
      if (tn.ms[k] < 0.995f * tn.ms[tn.best]) tn.best = k;  // (another placement has to win by 0.5 %: repeats agree to 0.1 %)
  }
  return UIS_OK;
}

// Step 4a: the per-decode tables onto the device, ev_begin, and the memory that must start out defined.
int upload_tables(DecodeCall& c) {
  uis_handle* h = c.h;
  const DevModel& m = h->m;
  const DecodeShape& s = c.shape;
  HIPCHK(hipMemcpyAsync(h->off.p, c.offsets, (size_t)(s.U + 1) * 8, hipMemcpyHostToDevice, h->stream));
  // (max_speakers: the caller's table, if there is one; k_init_state writes DecodeState::limit from it in every decode,
  // so that nothing depends on what an earlier call left there and an unbounded decode pays no copy)
  if (h->tables.limits.call_set)
    HIPCHK(hipMemcpyAsync(h->limit_in.p, h->tables.limits.data(), (size_t)s.U * 4, hipMemcpyHostToDevice, h->stream));
  // (uis_frame_bias: the whole table ahead of the first launch, also of a decode in several)
  if (h->tables.bias3.call_set && s.F > 0)
    HIPCHK(hipMemcpyAsync(h->bias3.p, h->tables.bias3.data(), (size_t)s.F * 24, hipMemcpyHostToDevice, h->stream));
  // (uis_min_turn: one value per utterance, where any of them sets a rule)
  if (s.turned)
    HIPCHK(hipMemcpyAsync(h->min_turn.p, h->tables.min_turn.data(), (size_t)s.U * 4, hipMemcpyHostToDevice, h->stream));
  // (uis_frame_speakers: likewise the whole tag table)
  if (h->tables.hint.call_set && s.F > 0)
    HIPCHK(hipMemcpyAsync(h->hint.p, h->tables.hint.data(), (size_t)s.F, hipMemcpyHostToDevice, h->stream));
  if (int rc = upload_log_tables(h->alpha, c.n_log, c.log_host, h->logblk.p, h->logden.p, h->stream)) return rc;
  if (s.wnd)
    HIPCHK(hipMemcpyAsync(h->bp_base.p, c.bp_base.data(), (size_t)(s.U + 1) * 8, hipMemcpyHostToDevice, h->stream));

  HIPCHK(hipEventRecord(h->ev_begin, h->stream));
  // never-written row descriptors must still name valid slots (step_tile in uis_kernels.hip)
  HIPCHK(hipMemsetAsync(h->rows.p, 0, (size_t)c.plan.rows_cap * sizeof(RnnRow), h->stream));
  HIPCHK(hipMemsetAsync(c.ctl, 0, kCtlWords * 4, h->stream));
  if (c.dbg && c.dbg_floats) HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(h->dbg_scores.p), 0x7f800000, c.dbg_floats, h->stream));
  if (c.rs)  // tiles a model does not have stay +0 in every row's partial sums
    HIPCHK(hipMemsetAsync(h->mse_tab.as<char>() + c.mse_tab_bytes, 0, c.mse_part_bytes, h->stream));
  c.d_x = (m.D != m.Dp && s.F > 0) ? h->xpad.as<float>() : c.d_frames;
  return UIS_OK;
}

// gi0 = W_ih0 x + b_ih0 and mse0 of n rows in each of `batches` batches (grid.z) with the 32-row x 16-tile workgroups:
// batch z starts z * stride rows behind the first, or -- `tab` -- at row tab[2 z] with tab[2 z + 1] rows.  `pipe`: the
// pipelined walk, instantiated for Dp 128 / 256 / 512 (every shape the planner splits a decode at is one of them).
int wide_input_proj(Launcher& lch, const DevModel& m, const float* x, float* gi0, float* mse0, long n, int batches, long stride,
                    const long* tab, bool pipe) {
  const dim3 wgrid((unsigned)((n + 31) / 32), (unsigned)((m.G / 16 + 15) / 16), (unsigned)batches);
  if (pipe && m.Dp == 128) LAUNCH(UIS_K_INPUT_PROJ, k_dense_input_proj_pipe<1>, wgrid, dim3(256), 0, m, x, gi0, n, stride, tab);
  else if (pipe && m.Dp == 256) LAUNCH(UIS_K_INPUT_PROJ, k_dense_input_proj_pipe<2>, wgrid, dim3(256), 0, m, x, gi0, n, stride, tab);
  else if (pipe && m.Dp == 512) LAUNCH(UIS_K_INPUT_PROJ, k_dense_input_proj_pipe<4>, wgrid, dim3(256), 0, m, x, gi0, n, stride, tab);
  else LAUNCH(UIS_K_INPUT_PROJ, k_dense_input_proj_wide, wgrid, dim3(256), 0, m, x, gi0, n);
  LAUNCH(UIS_K_INPUT_PROJ, k_mse0, dim3((unsigned)((n + 3) / 4), 1, (unsigned)batches), dim3(256), (size_t)5 * m.Dp * 4, m, x, mse0, n, stride, tab);
  return UIS_OK;
}

// Step 4: ingestion -- the frames onto the device, the input projection and the fresh-cluster MSEs.  Owns the cast
// team of a float64 list, the copy units and tables of a decode in several launches, and the way out: whichever way
// decode_once is left once begin() has run, both streams are drained first (the caller never gets its buffers back
// while the copy engine still reads them, and the tables below outlive their copies), and nobody is still inside the
// cast team when it goes away.
//   start()  the copy units; a float64 list's cast starts, in the order the frames are needed
//   begin()  everything a decode needs before its first launch: the whole list, or (split) its first slice
//   slice()  slice k of every utterance behind launch k - 1
struct Ingest {
  DecodeCall& c;
  uis_handle* const h;
  const DevModel& m;
  const bool uniform;    // utterances of equal length
  const int64_t uniN;    // the longest utterance: slice boundaries are frame indices inside an utterance
  const size_t pitch;    // (split, equal lengths: bytes between utterances, in the staging block and on the device)
  std::unique_ptr<CastTeam> team;
  CastPool* pool = nullptr;
  bool drain = false;
  // (split) what travels as ONE strided copy: a slice, or -- float64 lists, whose cast feeds the copies -- a piece of a
  // slice, so that a piece is on its way while the next one is cast; slice k = units [unit_first[k], unit_first[k + 1])
  struct CopyUnit { int64_t t0, t1; };
  std::vector<CopyUnit> units;
  std::vector<size_t> unit_first;
  std::vector<int64_t> cast_blocks_upto;  // blocks of the cast's order that end unit i
  std::vector<int64_t> unit_row0;         // (ragged) first row of unit i in the staging block (one more: the end)
  std::vector<long> scatter_tab_host;     // (ragged) k_scatter_rows' tables, unit after unit, {block row, stream row, rows} per utterance
  std::vector<long> split_tab_host;       // (ragged) the slices' batch tables

  explicit Ingest(DecodeCall& c_)
      : c(c_), h(c_.h), m(c_.h->m), uniform(!c_.shape.ragged), uniN(c_.shape.maxN), pitch((size_t)c_.shape.maxN * c_.h->m.D * 4) {}
  Ingest(const Ingest&) = delete;
  ~Ingest() {
    if (drain) { (void)hipStreamSynchronize(h->copy_stream); (void)hipStreamSynchronize(h->stream); }
    if (pool) pool->finish();
  }
  const std::vector<int64_t>& cuts() const { return c.plan.cuts; }
  int64_t slice_begin(size_t k) const { return k ? cuts()[k - 1] : 0; }
  int64_t slice_end(size_t k) const { return k < cuts().size() ? cuts()[k] : uniN; }

  void post(std::vector<std::pair<int64_t, int64_t>> order = {}, std::vector<int64_t> dst_rows = {}) {
    if (!h->cast_pool) h->cast_pool = new CastPool();
    team.reset(new CastTeam(h->src64, c.offsets, c.n_utt, m.D, c.shape.F, h->h_cast.as<float>(), std::move(order), std::move(dst_rows)));
    pool = static_cast<CastPool*>(h->cast_pool);
    pool->post(team.get());
  }

  void start() {
    if (!c.plan.split) return;
    for (size_t k = 0; k <= cuts().size(); ++k) {
      const int64_t t0 = slice_begin(k), t1 = slice_end(k);
      const int np = (k > 0 && h->src64) ? (int)std::max<int64_t>(1, std::min<int64_t>(8, (t1 - t0) / 64)) : 1;
      unit_first.push_back(units.size());
      for (int q = 0; q < np; ++q) units.push_back(CopyUnit{t0 + (t1 - t0) * q / np, t0 + (t1 - t0) * (q + 1) / np});
    }
    unit_first.push_back(units.size());
    if (!h->src64) return;
    // the cast starts NOW, in the order the frames are needed (every utterance's first slice, then the next ...), while
    // this thread is still busy with the decode's tables and memsets
    std::vector<std::pair<int64_t, int64_t>> order;
    std::vector<int64_t> dst_rows;
    int64_t cursor = 0;  // (ragged) next free row of the staging block
    for (size_t un = 0; un < units.size(); ++un) {
      unit_row0.push_back(cursor);
      for (int u = 0; u < c.n_utt; ++u) {
        const int64_t nu = c.offsets[u + 1] - c.offsets[u];
        const int64_t r0 = c.offsets[u] + std::min(units[un].t0, nu), r1 = c.offsets[u] + std::min(units[un].t1, nu);
        if (!uniform) {  // the scatter's table: {row in the block, row in the stream, rows}
          scatter_tab_host.push_back((long)cursor); scatter_tab_host.push_back((long)r0); scatter_tab_host.push_back((long)(r1 - r0));
        }
        for (int64_t r = r0; r < r1; r += CastTeam::kBlockRows) {
          order.emplace_back(r, std::min(r1, r + CastTeam::kBlockRows));
          if (!uniform) dst_rows.push_back(cursor + (r - r0));
        }
        cursor += r1 - r0;
      }
      cast_blocks_upto.push_back((int64_t)order.size());
    }
    unit_row0.push_back(cursor);
    post(std::move(order), std::move(dst_rows));
  }

  // once per decode: pad (only when D is not a multiple of 16), gi0 = W_ih0 x + b_ih0, mse0 of frames [f0, f1)
  int pre_chunk(Launcher& lch, int64_t f0, int64_t f1) {
    const long n = (long)(f1 - f0);
    if (m.D != m.Dp) {
      const long total = n * m.Dp;
      hipLaunchKernelGGL(k_pad_frames, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream,
                         c.d_frames + (size_t)f0 * m.D, h->xpad.as<float>() + (size_t)f0 * m.Dp, n, m.D, m.Dp);
      HIPCHK(hipGetLastError());
    }
    const float* xin = c.d_x + (size_t)f0 * m.Dp;
    float* gout = h->gi0.as<float>() + (size_t)f0 * m.G;
    if (n >= UIS_PROJ_WIDE_ROWS)  // enough rows to fill the device with 32-row x 16-tile workgroups
      return wide_input_proj(lch, m, xin, gout, h->mse0.as<float>() + f0, n, 1, 0L, nullptr,
                             !(c.opts->flags & UIS_FLAG_SMALL_TILES));  // (the flag keeps the plain walk for A/B runs)
    return plain_input_proj(lch, m, xin, gout, h->mse0.as<float>() + f0, n);
  }
  // slice k = rows [t0, t1) of every utterance: input projection and fresh-cluster MSE, the utterances as batches
  // (uniform: batch z starts z * uniN rows behind the first; ragged: the slice's table of {first row, rows} per utterance)
  int pre_rows(Launcher& lch, size_t k) {
    const int64_t t0 = slice_begin(k);
    if (uniform)
      return wide_input_proj(lch, m, c.d_x + (size_t)t0 * m.Dp, h->gi0.as<float>() + (size_t)t0 * m.G, h->mse0.as<float>() + t0,
                             (long)(slice_end(k) - t0), c.shape.U, (long)uniN, nullptr, true);
    return wide_input_proj(lch, m, c.d_x, h->gi0.as<float>(), h->mse0.as<float>(), (long)(slice_end(k) - t0), c.shape.U, (long)uniN,
                           h->split_tab.as<long>() + k * (size_t)c.shape.U * 2, true);
  }
  // copy unit `un` of every utterance, host -> device
  int copy_rows(size_t un) {
    if (team) team->wait_blocks(cast_blocks_upto[un]);
    if (uniform) {
      const int64_t t0 = units[un].t0, t1 = units[un].t1;
      HIPCHK(hipMemcpy2DAsync(const_cast<float*>(c.d_frames) + (size_t)t0 * m.D, pitch, c.h_frames + (size_t)t0 * m.D, pitch,
                              (size_t)(t1 - t0) * m.D * 4, (size_t)c.shape.U, hipMemcpyHostToDevice, h->copy_stream));
      return UIS_OK;
    }
    // ragged (float64 lists only): the unit is one block of the staging buffer -> the same rows of the device's block,
    // then every utterance's part to its place in the frame stream (on the copy stream too: ordered behind the copy)
    const int64_t r0 = unit_row0[un], r1 = unit_row0[un + 1];
    if (r1 > r0) {
      HIPCHK(hipMemcpyAsync(h->stage.as<float>() + (size_t)r0 * m.D, c.h_frames + (size_t)r0 * m.D, (size_t)(r1 - r0) * m.D * 4,
                            hipMemcpyHostToDevice, h->copy_stream));
      const long max_rows = (long)(units[un].t1 - units[un].t0);
      hipLaunchKernelGGL(k_scatter_rows, dim3((unsigned)std::min<long>(64, (max_rows * (m.D / 4) + 255) / 256), (unsigned)c.shape.U), dim3(256), 0,
                         h->copy_stream, h->stage.as<float>(), const_cast<float*>(c.d_frames), h->scatter_tab.as<long>() + un * (size_t)c.shape.U * 3, m.D);
      HIPCHK(hipGetLastError());
    }
    return UIS_OK;
  }
  // the copy units of slice k, then its projection on lch's stream once they have landed
  int slice(Launcher& lch, size_t k) {
    int rc;
    for (size_t un = unit_first[k]; un < unit_first[k + 1]; ++un)
      if ((rc = copy_rows(un))) return rc;
    HIPCHK(hipEventRecord(h->h2d_done[k], h->copy_stream));
    HIPCHK(hipStreamWaitEvent(lch.stream, h->h2d_done[k], 0));
    return pre_rows(lch, k);
  }

  int begin(Launcher& lch) {
    const int64_t F = c.shape.F;
    const int U = c.shape.U;
    int rc;
    drain = true;  // from here on DMA from the caller's (or the pinned staging) memory may be in flight
    if (c.plan.split) {
      if ((rc = grow_events(h->h2d_done, cuts().size() + 1))) return rc;
      HIPCHK(hipStreamWaitEvent(h->copy_stream, h->ev_begin, 0));
      if (!uniform) {  // the slices' batch tables: {first row, rows} per utterance and slice
        std::vector<long>& tab = split_tab_host;
        tab.assign((cuts().size() + 1) * (size_t)U * 2, 0L);
        for (size_t k = 0; k <= cuts().size(); ++k) {
          for (int u = 0; u < U; ++u) {
            const int64_t nu = c.offsets[u + 1] - c.offsets[u], a = std::min(slice_begin(k), nu);
            tab[(k * U + u) * 2] = (long)(c.offsets[u] + a);
            tab[(k * U + u) * 2 + 1] = (long)(std::min(slice_end(k), nu) - a);
          }
        }
        HIPCHK(hipMemcpyAsync(h->split_tab.p, tab.data(), tab.size() * sizeof(long), hipMemcpyHostToDevice, h->stream));
        // (the scatter runs on the copy stream: its tables go up on that stream, ahead of the first block)
        HIPCHK(hipMemcpyAsync(h->scatter_tab.p, scatter_tab_host.data(), scatter_tab_host.size() * sizeof(long), hipMemcpyHostToDevice,
                              h->copy_stream));
      }
      return slice(lch, 0);
    }
    if (F > 0 && c.h_frames) {
      // Host frames (uis_decode) arrive in chunks on the copy stream; chunk i's kernels overlap the
      // H2D of chunk i+1 (true overlap needs pinned host memory, uis_host_alloc).
      const int n_chunks = (int)std::max<int64_t>(1, std::min<int64_t>(UIS_H2D_CHUNKS, F / UIS_H2D_MIN_FRAMES));
      if ((rc = grow_events(h->h2d_done, (size_t)n_chunks))) return rc;
      HIPCHK(hipStreamWaitEvent(h->copy_stream, h->ev_begin, 0));
      // float64 utterances: cast into the pinned staging buffer by the handle's pool (and this thread),
      // piece p + 1 while piece p copies / projects.  A projection chunk then travels in several pieces,
      // so that the first copy starts after an eighth of the cast, not half of it.
      if (h->src64) post();
      const int pieces = team ? (int)std::max<int64_t>(1, std::min<int64_t>(UIS_F64_PIECES, (F / n_chunks) / 1024)) : 1;
      for (int ch = 0; ch < n_chunks; ++ch) {
        const int64_t f0 = F * ch / n_chunks, f1 = F * (ch + 1) / n_chunks;
        for (int pc = 0; pc < pieces; ++pc) {
          const int64_t g0 = f0 + (f1 - f0) * pc / pieces, g1 = f0 + (f1 - f0) * (pc + 1) / pieces;
          if (team) team->wait_rows(g1);
          HIPCHK(hipMemcpyAsync(const_cast<float*>(c.d_frames) + (size_t)g0 * m.D, c.h_frames + (size_t)g0 * m.D,
                                (size_t)(g1 - g0) * m.D * 4, hipMemcpyHostToDevice, h->copy_stream));
        }
        HIPCHK(hipEventRecord(h->h2d_done[ch], h->copy_stream));
        HIPCHK(hipStreamWaitEvent(h->stream, h->h2d_done[ch], 0));
        if ((rc = pre_chunk(lch, f0, f1))) return rc;
      }
      return UIS_OK;
    }
    return F > 0 ? pre_chunk(lch, 0, F) : UIS_OK;
  }
};

// Step 5: every group's view of the shared buffers (pointers offset to the group's first utterance).
void build_group_states(DecodeCall& c) {
  uis_handle* h = c.h;
  const DevModel& m = h->m;
  const DecodeShape& s = c.shape;
  const int B = s.B, Kmax = s.Kmax, S = s.S, L = s.L;
  const size_t NC = (size_t)s.NC, rows_per_utt = (size_t)(L == 1 ? B : s.NC);
  for (int g = 0; g < s.G; ++g) {
    GroupPlan& gp = c.groups[g];
    DecodeState& st = gp.st;
    const size_t u0 = (size_t)gp.u0;
    st.U = gp.U; st.B = B; st.Kmax = Kmax; st.S = S; st.L = L; st.tau = c.tau; st.flags = c.opts->flags | (c.knobs.agent_flags ? UIS_FLAG_AGENT_FLAGS : 0u); st.wnd = s.wnd ? 1 : 0;
    st.max_rows = (int)((size_t)gp.U * rows_per_utt);
    st.off = h->off.as<int64_t>() + u0;
    st.utt_step = h->utt_step.as<int32_t>() + u0;
    st.overflow = h->overflow.as<int32_t>() + u0;
    st.limit = h->limit.as<int32_t>() + u0;
    st.limit_in = h->tables.limits.call_set ? h->limit_in.as<int32_t>() + u0 : nullptr;
    st.bias3 = h->tables.bias3.call_set ? h->bias3.as<double>() : nullptr;  // (indexed by the packed frame, like mse0)
    st.hint = h->tables.hint.call_set ? h->hint.as<uint8_t>() : nullptr;   // (likewise)
    st.min_turn = c.shape.turned ? h->min_turn.as<int32_t>() + u0 : nullptr;
    st.x = c.d_x; st.gi0 = h->gi0.as<float>(); st.mse0 = h->mse0.as<float>();
    st.logblk = h->logblk.as<double>(); st.logden = h->logden.as<double>();
    st.pool_mean = h->pool_mean.as<float>() + u0 * S * m.Dp;
    st.pool_hid = h->pool_hid.as<float>() + u0 * S * m.depth * m.Hp;
    st.pool_cnt = h->pool_cnt.as<int32_t>() + u0 * S;
    // beam tables: groups back to back, each laid out [2][U_g][...]
    st.beam_n = h->beam_n.as<int32_t>() + 2 * u0;
    st.beam_K = h->beam_K.as<int32_t>() + 2 * u0 * B;
    st.beam_last = h->beam_last.as<int32_t>() + 2 * u0 * B;
    st.beam_sum = h->beam_sum.as<int32_t>() + 2 * u0 * B;
    st.beam_score = h->beam_score.as<float>() + 2 * u0 * B;
    st.beam_slot = h->beam_slot.as<int32_t>() + 2 * u0 * B * Kmax;
    st.beam_blk = h->beam_blk.as<int32_t>() + 2 * u0 * B * Kmax;
    st.bp = h->bp.as<uint32_t>();
    st.rows = h->rows.as<RnnRow>() + u0 * rows_per_utt + 48 * (size_t)g;
    st.nrows = h->nrows.as<int32_t>() + 2 * g;
    st.gi_up = h->gi_up.as<float>() + (m.depth > 1 ? (u0 * rows_per_utt + 48 * (size_t)g) * m.G : 0);
    st.a1 = h->a1.as<float>() + (u0 * rows_per_utt + 48 * (size_t)g) * m.Hp;
    st.counters = h->counters.as<unsigned long long>() + 4 * g;
    st.utt_nrows = h->utt_nrows.as<int32_t>() + 2 * u0;
    st.hst = c.plan.hst ? h->hst.as<float>() : nullptr;
    st.step0 = 0; st.step1 = 0; st.resume = h->resume.as<unsigned char>(); st.resume_stride = 0;
    st.hst_elems = (size_t)c.plan.rows_cap * m.Hp;
    st.dbg_scores = c.dbg ? h->dbg_scores.as<float>() + 0 : nullptr;  // (one group: groups would need their own utterance offset)
    wire_cluster_ctl(st, c.ctl, c.plan.clustered() ? &c.plan : nullptr);
    if (c.rs) {  // (one group)
      st.mse_tab = h->mse_tab.as<float>();
      st.mse_part = reinterpret_cast<float*>(h->mse_tab.as<char>() + c.mse_tab_bytes);
    }
    if (s.wnd) {  // level buffers: groups back to back, each [2][U_g][NC]...
      st.NC = (int)NC;
      st.lv_n = h->lv_n.as<int32_t>() + 2 * u0;
      st.lv_K = h->lv_K.as<int32_t>() + 2 * u0 * NC;
      st.lv_last = h->lv_last.as<int32_t>() + 2 * u0 * NC;
      st.lv_sum = h->lv_sum.as<int32_t>() + 2 * u0 * NC;
      st.lv_score = h->lv_score.as<float>() + 2 * u0 * NC;
      st.lv_origin = h->lv_origin.as<int32_t>() + 2 * u0 * NC;
      st.lv_path = h->lv_path.as<int16_t>() + 2 * u0 * NC * L;
      st.lv_slot = h->lv_slot.as<int32_t>() + 2 * u0 * NC * Kmax;
      st.lv_blk = h->lv_blk.as<int32_t>() + 2 * u0 * NC * Kmax;
      st.scratch = h->scratch.as<unsigned char>() + u0 * c.wsl.total;
      st.scratch_stride = c.wsl.total;
      st.bp16 = h->bp16.as<uint16_t>();
      st.bp_base = h->bp_base.as<int64_t>() + u0;
    }
  }
}

// The step kernels of a group as a captured graph of UIS_GRAPH_STEPS steps, launched as often as the group needs
// (the graph is kept while the group's state and LDS size stay what they were).
int launch_graph(DecodeCall& c, int g, Launcher& gl) {
  uis_handle* h = c.h;
  const GroupPlan& gp = c.groups[g];
  GraphCache& gc = h->gcache[g];
  const bool same = gc.exec && gc.lds == c.plan.lds && memcmp(&gc.st, &gp.st, sizeof(DecodeState)) == 0;
  if (!same) {
    if (gc.exec) { (void)hipGraphExecDestroy(gc.exec); gc.exec = nullptr; }
    hipGraph_t graph = nullptr;
    HIPCHK(hipStreamBeginCapture(gl.stream, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue_steps(h, gl, gp.st, c.plan.lds, UIS_GRAPH_STEPS);
    hipError_t ce = hipStreamEndCapture(gl.stream, &graph);
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (ce != hipSuccess) return fail(UIS_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
    ce = hipGraphInstantiate(&gc.exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ce != hipSuccess) { gc.exec = nullptr; return fail(UIS_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ce)); }
    gc.st = gp.st; gc.lds = c.plan.lds;
  }
  const int64_t nlaunch = (gp.maxT + UIS_GRAPH_STEPS - 1) / UIS_GRAPH_STEPS;  // the tail steps are no-ops
  for (int64_t i = 0; i < nlaunch; ++i) HIPCHK(hipGraphLaunch(gc.exec, gl.stream));
  return UIS_OK;
}

// Step 6: the decode of group g on its own stream, by the plan's path, and its back-trace.
int launch_group(DecodeCall& c, Ingest& ing, int g) {
  uis_handle* h = c.h;
  const DevModel& m = h->m;
  const DecodeShape& s = c.shape;
  const DecodePlan& plan = c.plan;
  GroupPlan& gp = c.groups[g];
  hipStream_t sg = h->gstreams[g];
  Launcher lch{h, sg, c.profile};  // LAUNCH() below targets this group's stream
  int rc;
  HIPCHK(hipStreamWaitEvent(sg, h->ev_pre, 0));
  LAUNCH(-1, k_init_state, dim3((gp.U + 255) / 256), dim3(256), 0, gp.st);
  if (plan.clustered()) {
    // h1 (of every layer) into the extra slot, then ONE launch for every step of every utterance -- or (split) one
    // per slice of the frames, the next slice arriving behind it
    HIPCHK(hipMemcpyAsync(gp.st.pool_hid + (size_t)s.U * s.S * m.depth * m.Hp, m.h1, (size_t)m.depth * m.Hp * 4, hipMemcpyDeviceToDevice, sg));
    const std::vector<int64_t>& cuts = plan.cuts;
    for (size_t k = 0; k <= cuts.size(); ++k) {
      if (k > 0) {
        // slice k of every utterance: cast (float64 lists), one strided copy, projection -- behind launch k - 1
        if ((rc = ing.slice(lch, k))) return rc;
        // (k_decode_big<WS> counts its barriers and rows from zero in every launch; the abort word and the XCC ids stay)
        if (!c.rs) HIPCHK(hipMemsetAsync(c.ctl + 32, 0, (kCtlWords - 32) * 4, sg));
      }
      if (plan.split) {
        gp.st.step0 = k ? (int)cuts[k - 1] - 1 : 0;
        gp.st.step1 = k < cuts.size() ? (int)cuts[k] - 1 : 0;
      }
      if ((rc = c.rs ? launch_rs_kernel(lch, c.rs_kern, h->n_cu, plan.ncl, plan.lds, m, gp.st, h->bp.cap)
                     : launch_cluster_kernel(lch, c.cluster_kern, h->n_cu, plan.ncl, plan.lds, m, gp.st))) return rc;
    }
  } else if (plan.path == DecodePath::SMALL) {
    DecodeKernel kern = s.L == 1 ? &k_decode_small<false> : &k_decode_small<true>;
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
    LAUNCH(UIS_K_GRU, kern, dim3(gp.U), dim3(512), plan.lds, m, gp.st);
  } else if (plan.path == DecodePath::GRAPH && gp.maxT >= UIS_GRAPH_STEPS) {
    if ((rc = launch_graph(c, g, lch))) return rc;
  } else {
    const int64_t nsteps = gp.maxT + (gp.maxT & 1);
    for (int64_t s0 = 0; s0 < nsteps; s0 += 2)
      if ((rc = enqueue_steps(h, lch, gp.st, plan.lds, 2))) return rc;
  }
  float* const scores = c.d_scores ? c.d_scores + gp.u0 : nullptr;
  float* const beam_scores = h->beam_scores_out.as<float>() + (size_t)gp.u0 * s.B;
  if (!s.wnd) LAUNCH(UIS_K_BACKTRACE, k_backtrace, dim3(gp.U), dim3(64), (size_t)64 * s.B, gp.st, c.d_labels, scores, beam_scores);
  else LAUNCH(UIS_K_BACKTRACE, k_backtrace_window, dim3((gp.U + 63) / 64), dim3(64), 0, gp.st, c.d_labels, scores, beam_scores);
  HIPCHK(hipEventRecord(h->gdone[g], sg));
  return UIS_OK;
}

// Step 7: what the decode left behind -- its counters, flags and final beam to the host, uis_stats, and the state
// uis_last_decode_nbest reads.
int collect_results(DecodeCall& c) {
  uis_handle* h = c.h;
  const DecodeShape& s = c.shape;
  const int U = s.U, G = s.G;
  std::vector<unsigned long long> counters((size_t)UIS_MAX_GROUPS * 4, 0ull);
  HIPCHK(hipMemcpyAsync(counters.data(), h->counters.p, (size_t)G * 4 * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(h->last_overflow.data(), h->overflow.p, (size_t)U * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(h->last_beam_scores.data(), h->beam_scores_out.p, (size_t)U * s.B * 4, hipMemcpyDeviceToHost,
                        h->stream));
  uint32_t abort_word = 0;
  HIPCHK(hipMemcpyAsync(&abort_word, c.ctl + 16, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (c.dbg) h->dbg_floats = c.dbg_floats;
  if (abort_word) {
    h->inlaunch_failed = true;
    return fail(UIS_ERR_HIP, abort_word == 2 ? "workgroup cluster not placed on one XCD (in-launch barrier path)"
                                             : "in-launch barrier timed out");
  }
  int rc;
#if defined(UIS_SELECT_TIMING) || defined(UIS_RESIDENT_PROBE) || defined(UIS_RS_COUNT_PATHS) || defined(UIS_RESIDENT_TIMING)
  if ((rc = report_diagnostics(h, c.plan, U, s.maxT, s.L))) return rc;
#endif
  if ((rc = ctl_record(c))) return rc;
  const int n_over = count_cluster_cap(h->last_overflow);
  int n_level = 0;
  for (int u = 0; u < U; ++u) n_level += (h->last_overflow[u] & 2) != 0;  // look_ahead >= 2: an intermediate level was full
  if (uis_stats* stats = c.stats) {
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, h->ev_begin, h->ev_end));
    stats->n_steps = (int32_t)s.maxT;
    stats->decode_ms = ms;
    for (int g = 0; g < G; ++g) {
      stats->rnn_rows += (int64_t)counters[4 * g + 0];
      stats->rnn_rows_nodedup += (int64_t)counters[4 * g + 1];
      stats->candidates += (int64_t)counters[4 * g + 2];
      stats->max_clusters_seen = std::max(stats->max_clusters_seen, (int32_t)counters[4 * g + 3]);
    }
    stats->n_overflow = n_over;
    stats->n_streams = G;
    stats->decode_kernel = c.plan.decode_kernel;
    stats->decode_launches = c.plan.one_launch() ? (int)c.plan.cuts.size() + 1 : 0;
    if (c.profile) {
      for (size_t i = 0; i + 1 < h->prof.used; i += 2) {
        float t = 0.0f;
        HIPCHK(hipEventElapsedTime(&t, h->prof.ev[i], h->prof.ev[i + 1]));
        const int cl = h->prof.cls[i / 2];
        if (cl < 0) continue;
        stats->kernel_ms[cl] += t;
        stats->kernel_launches[cl] += 1;
      }
    }
  }
  if (n_level)
    return fail(UIS_ERR_UNSUPPORTED,
                std::to_string(n_level) + " utterance(s) had more than " + std::to_string((long long)s.NC) +
                    " live assignment prefixes inside a look-ahead window (beam_size * clusters ^ (look_ahead - 1)); "
                    "a larger max_clusters cannot help: lower look_ahead or beam_size");
  // the back-pointers and the final beam of every group stay where they are until the next decode: uis_last_decode_nbest
  h->nb_groups.clear();
  for (int g = 0; g < G; ++g) h->nb_groups.push_back(uis_handle::NbestGroup{c.groups[g].st, c.groups[g].u0});
  h->nb_offsets.assign(c.offsets, c.offsets + U + 1);
  h->nb_B = s.B; h->nb_wnd = s.wnd; h->nb_valid = true;
  return cluster_cap_status(n_over, s.Kmax);
}

int decode_once(uis_handle* h, const float* d_frames, const int64_t* offsets, int32_t n_utt,
                const uis_decode_opts* opts, int32_t* d_labels, float* d_scores, uis_stats* stats,
                const float* h_frames = nullptr) {
  if (!h || !offsets || !opts || n_utt < 0) return fail(UIS_ERR_INVALID_ARG, "null handle/offsets/opts or negative n_utt");
  DecodeCall c{h, d_frames, offsets, n_utt, opts, d_labels, d_scores, stats, h_frames, read_knobs()};
  int rc;
  if ((rc = derive_shape(c)) || c.shape.U == 0) return rc;
  if ((rc = plan_and_place(c))) return rc;
  ctl_choose(c);
  Launcher lch{h, h->stream, c.profile};
  Ingest ing(c);  // (declared after `c`: its way out drains the streams while c's tables are still there)
  ing.start();
  if ((rc = upload_tables(c))) return rc;
  if ((rc = ing.begin(lch))) return rc;
  HIPCHK(hipEventRecord(h->ev_pre, h->stream));
  build_group_states(c);
  if (c.plan.clustered() && !c.cluster_kern && !c.rs_kern) return fail(UIS_ERR_HIP, "no one-launch kernel instantiated for this shape");
  for (int g = 0; g < c.shape.G; ++g)
    if ((rc = launch_group(c, ing, g))) return rc;
  for (int g = 0; g < c.shape.G; ++g) HIPCHK(hipStreamWaitEvent(h->stream, h->gdone[g], 0));
  HIPCHK(hipEventRecord(h->ev_end, h->stream));
  return collect_results(c);
}

// One decode; if the one-launch path was chosen automatically and its placement / barrier checks
// failed, repeat on the launch-per-step path and stay there for this handle.
int decode_impl(uis_handle* h, const float* d_frames, const int64_t* offsets, int32_t n_utt,
                const uis_decode_opts* opts, int32_t* d_labels, float* d_scores, uis_stats* stats,
                const float* h_frames = nullptr) {
  if (h) h->inlaunch_failed = false;
  int rc = decode_once(h, d_frames, offsets, n_utt, opts, d_labels, d_scores, stats, h_frames);
  if (rc == UIS_ERR_HIP && h && h->inlaunch_failed && opts &&
      !(opts->flags & UIS_FLAG_RESIDENT)) {
    // (the frames, if they came from the host, travel again: a decode in several launches that was refused at its
    // first launch has only the first slice on the device)
    h->resident_off = true;
    rc = decode_once(h, d_frames, offsets, n_utt, opts, d_labels, d_scores, stats, h_frames);
  }
  return rc;
}

}  // namespace

UIS_EXPORT int32_t uis_abi_version(void) { return UIS_ABI_VERSION; }
UIS_EXPORT int32_t uis_numerics_version(void) { return UIS_NUMERICS_VERSION; }
UIS_EXPORT uint32_t uis_build_flags(void) { return 0; }

UIS_EXPORT int32_t uis_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

UIS_EXPORT const char* uis_last_error(void) { return g_err.c_str(); }

// For the other translation units of the library (uis_train.hip): their failures land in the
// same thread-local message uis_last_error() returns.
int uis_internal_fail(int code, const std::string& msg) { return fail(code, msg); }

// A session's memory back to the device and the host, and the session closed (uis_stream_end, a uis_stream_begin that
// fails half-way, uis_destroy).
static void stream_free(uis_handle* h) {
  uis_handle::Stream& ss = h->stream_state;
  static_cast<StreamMem&>(ss) = StreamMem{};
  ss.persist = false; ss.pm_running = false;
  ss.active = false;
  ss.have.clear();
}

UIS_EXPORT void uis_destroy(uis_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream_state.pm_running) {  // tell the resident launch to leave before waiting for the stream
    pm_ring(h->stream_state, h->stream_state.pm_seq + 1, UIS_PM_QUIT, 0);
    h->stream_state.pm_running = false;
  }
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  stream_free(h);
  for (void* p : h->model_allocs) (void)hipFree(p);
  static_cast<HandleMem&>(*h) = HandleMem{};  // (every buffer, before the streams they were used on go)
  for (hipEvent_t e : h->prof.ev) (void)hipEventDestroy(e);
  if (h->ev_begin) (void)hipEventDestroy(h->ev_begin);
  if (h->ev_end) (void)hipEventDestroy(h->ev_end);
  if (h->ev_pre) (void)hipEventDestroy(h->ev_pre);
  if (h->ev_producer) (void)hipEventDestroy(h->ev_producer);
  for (GraphCache& gc : h->gcache) if (gc.exec) (void)hipGraphExecDestroy(gc.exec);
  for (hipEvent_t e : h->gdone) (void)hipEventDestroy(e);
  for (hipStream_t sg : h->gstreams) { (void)hipStreamSynchronize(sg); (void)hipStreamDestroy(sg); }
  for (hipEvent_t e : h->h2d_done) (void)hipEventDestroy(e);
  if (h->cast_pool) { delete static_cast<CastPool*>(h->cast_pool); h->cast_pool = nullptr; }
  if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

UIS_EXPORT int32_t uis_create(const uis_model_desc* d, int32_t device, uis_handle** out) {
  if (!d || !out) return fail(UIS_ERR_INVALID_ARG, "null desc/out");
  *out = nullptr;
  const int D = d->observation_dim, H = d->rnn_hidden_size, depth = d->rnn_depth;
  if (D < 1 || H < 1 || depth < 1 || depth > UIS_MAX_DEPTH)
    return fail(UIS_ERR_INVALID_ARG, "observation_dim, rnn_hidden_size >= 1 and 1 <= rnn_depth <= 8 required");
  if (!(d->transition_bias > 0.0 && d->transition_bias < 1.0))
    return fail(UIS_ERR_INVALID_ARG, "transition_bias must be in (0, 1) (the reference takes its log)");
  if (!(d->crp_alpha > 0.0)) return fail(UIS_ERR_INVALID_ARG, "crp_alpha must be > 0");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(UIS_ERR_NO_DEVICE, "no HIP device visible; this decoder has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(UIS_ERR_NO_DEVICE, "device index out of range");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(UIS_ERR_NO_DEVICE, "hipGetDeviceProperties failed");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(UIS_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
  if (hipSetDevice(device) != hipSuccess) return fail(UIS_ERR_NO_DEVICE, "hipSetDevice failed");

  uis_handle* h = new uis_handle();
  h->device = device;
  h->alpha = d->crp_alpha;
  if (hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) h->n_cu = 0;
  auto bail = [&](int rc) { uis_destroy(h); return rc; };
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking) != hipSuccess)
    return bail(fail(UIS_ERR_HIP, "stream create failed"));
  if (hipEventCreate(&h->ev_begin) != hipSuccess || hipEventCreate(&h->ev_end) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_pre, hipEventDisableTiming) != hipSuccess)
    return bail(fail(UIS_ERR_HIP, "event create failed"));
  DevModel& m = h->m;
  m.D = D; m.H_units = H; m.depth = depth;
  m.Dp = round_up(D, 16); m.Hp = round_up(H, 16);
  // The one-launch cluster kernels exist for padded hidden sizes 256 / 512 and observation dims 128 / 256 /
  // 512.  Padding further than to 16 is free of numerical consequences exactly where it keeps the canonical
  // K-segment length q = ceil(blocks / 8) (uis_numerics.h: the extra blocks are zeros inside the last
  // segments, empty segments add +0.0f either way; the MSE's sixteen tile accumulators take zero tiles):
  // hidden sizes 65 .. 256 and 385 .. 512, observation dims up to 256 and 385 .. 512 -- so those models
  // (rnn_depth 1) get the kernels' shapes instead of the launch-per-step path.
  HidMap hmap;
  if (!getenv("UIS_PAD_TO_16_ONLY")) {  // (any rnn_depth: the upper layers' K axis is the hidden size too)
    const int qh = (m.Hp / 16 + UIS_KSPLIT - 1) / UIS_KSPLIT, qd = (m.Dp / 16 + UIS_KSPLIT - 1) / UIS_KSPLIT;
    // (round 6) hidden sizes 257 .. 384 have segments of three k-blocks: into the 512 shape with a zero block behind
    // every segment (HidMap) -- they ran a launch per step before (UIS_NO_SEGMENT_PADDING=1: still do)
    const bool seg3 = qh == 3 && !getenv("UIS_NO_SEGMENT_PADDING");
    const int hp = (qh == 1 && H > 64) ? 128 : qh == 2 ? 256 : (qh == 4 || seg3) ? 512 : 0;  // (up to 64: k_decode_small's)
    const int dp = m.Dp <= 128 ? 128 : qd == 2 ? 256 : qd == 4 ? 512 : 0;
    if (hp && dp) {
      m.Hp = hp; m.Dp = dp;
      if (seg3) {
        hmap.seg = 3 * 16; hmap.seg_p = 4 * 16;
        m.H_units = m.Hp;  // (the kernels' `unit < H_units` masks: the model's units are spread over the whole padded vector; the rest stay 0 by themselves)
      }
    }
  }
  h->hid_map_seg = hmap.seg; h->hid_map_seg_p = hmap.seg_p; h->H_model = H;
  {  // the model fingerprint's hash: every parameter in the descriptor's order, on the host
    uint64_t fp = 0;
    auto mix = [&](const void* p, size_t bytes) { fp = uis_blob_hash(p, bytes, fp); };
    for (int l = 0; l < depth; ++l) {
      mix(d->gru_weight_ih[l], (size_t)3 * H * (l == 0 ? D : H) * 4);
      mix(d->gru_weight_hh[l], (size_t)3 * H * H * 4);
      mix(d->gru_bias_ih[l], (size_t)3 * H * 4);
      mix(d->gru_bias_hh[l], (size_t)3 * H * 4);
    }
    mix(d->linear_mean1_weight, (size_t)H * H * 4);
    mix(d->linear_mean1_bias, (size_t)H * 4);
    mix(d->linear_mean2_weight, (size_t)D * H * 4);
    mix(d->linear_mean2_bias, (size_t)D * 4);
    mix(d->rnn_init_hidden, (size_t)depth * H * 4);
    mix(d->sigma2, (size_t)D * 4);
    const double priors[2] = {d->transition_bias, d->crp_alpha};
    mix(priors, sizeof(priors));
    h->model_hash = fp;
  }
  m.G = 3 * m.Hp;
  m.lp_stay = std::log(1.0 - d->transition_bias);  // np.log(1 - transition_bias), uisrnn.py:416
  m.lp_sw = std::log(d->transition_bias);
  m.l_alpha = std::log(d->crp_alpha);
  m.lp_new = m.lp_sw + m.l_alpha;
  int rc;
  for (int l = 0; l < depth; ++l) {
    const int K = l == 0 ? D : H, Kp = l == 0 ? m.Dp : m.Hp;
    if ((rc = upload(h, tile_weights(d->gru_weight_ih[l], 3, H, m.Hp, K, Kp, hmap, l == 0 ? HidMap() : hmap), &m.wih[l]))) return bail(rc);
    if ((rc = upload(h, tile_weights(d->gru_weight_hh[l], 3, H, m.Hp, H, m.Hp, hmap, hmap), &m.whh[l]))) return bail(rc);
    if ((rc = upload(h, pad_bias(d->gru_bias_ih[l], 3, H, m.Hp, hmap), &m.bih[l]))) return bail(rc);
    if ((rc = upload(h, pad_bias(d->gru_bias_hh[l], 3, H, m.Hp, hmap), &m.bhh[l]))) return bail(rc);
  }
  if ((rc = upload(h, tile_weights(d->linear_mean1_weight, 1, H, m.Hp, H, m.Hp, hmap, hmap), &m.w1))) return bail(rc);
  if ((rc = upload(h, pad_bias(d->linear_mean1_bias, 1, H, m.Hp, hmap), &m.b1))) return bail(rc);
  if ((rc = upload(h, tile_weights(d->linear_mean2_weight, 1, D, m.Dp, H, m.Hp, HidMap(), hmap), &m.w2))) return bail(rc);
  if ((rc = upload(h, pad_bias(d->linear_mean2_bias, 1, D, m.Dp), &m.b2))) return bail(rc);
  std::vector<float> wgt(m.Dp, 0.0f);
  for (int i = 0; i < D; ++i) wgt[i] = 1.0f / (2.0f * d->sigma2[i]);  // 1 / (2 * sigma2), uisrnn.py:414
  if ((rc = upload(h, wgt, &m.wgt))) return bail(rc);
  std::vector<float> hinit((size_t)depth * m.Hp, 0.0f);
  for (int l = 0; l < depth; ++l)
    for (int j = 0; j < H; ++j) hinit[(size_t)l * m.Hp + hmap(j)] = d->rnn_init_hidden[(size_t)l * H + j];
  const float* d_hinit = nullptr;
  if ((rc = upload(h, hinit, &d_hinit))) return bail(rc);
  if ((rc = upload(h, std::vector<float>(m.Dp, 0.0f), &m.m0))) return bail(rc);
  if ((rc = upload(h, std::vector<float>((size_t)depth * m.Hp, 0.0f), &m.h1))) return bail(rc);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_select_fast), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_wt_gru<32>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_wt_gru<32, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_wt_head<32, 1, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_wt_head<32, 2, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_window<256>), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_window<UIS_WINDOW_WIDE_NT>), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_select), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (e != hipSuccess) return bail(fail(UIS_ERR_HIP, std::string("hipFuncSetAttribute(k_select): ") + hipGetErrorString(e)));
  if ((rc = bootstrap_constants(h, d_hinit))) return bail(rc);
  *out = h;
  return UIS_OK;
}

// The setters of the per-call tables: validation and conversion are uis_call_tables.h's.
UIS_EXPORT int32_t uis_decode_limits(uis_handle* h, const int32_t* limits, int32_t n_utt) {
  if (!h) return fail(UIS_ERR_INVALID_ARG, "null handle");
  return table_status(h->tables.set_limits(limits, n_utt));
}

UIS_EXPORT int32_t uis_min_turn(uis_handle* h, const int32_t* min_turn, int32_t n_utt) {
  if (!h) return fail(UIS_ERR_INVALID_ARG, "null handle");
  return table_status(h->tables.set_min_turn(min_turn, n_utt));
}

UIS_EXPORT int32_t uis_frame_speakers(uis_handle* h, const uint8_t* tags, int64_t n_frames) {
  if (!h) return fail(UIS_ERR_INVALID_ARG, "null handle");
  return table_status(CallTables::set_tags(h->tables.hint, tags, n_frames));
}

UIS_EXPORT int32_t uis_stream_speakers(uis_handle* h, const uint8_t* tags, int64_t n_frames) {
  if (int rc = begin_call(h, "uis_stream_speakers", UIS_RULE_STREAM_OTHER)) return rc;
  if (!h) return fail(UIS_ERR_INVALID_ARG, "null handle");
  return table_status(CallTables::set_tags(h->tables.stream_tags, tags, n_frames));
}

UIS_EXPORT int32_t uis_frame_bias(uis_handle* h, const double* bias, int64_t n_frames) {
  if (!h) return fail(UIS_ERR_INVALID_ARG, "null handle");
  const DevModel& m = h->m;
  const double model3[3] = {m.lp_stay, m.lp_sw, m.lp_new};
  return table_status(h->tables.set_bias(bias, n_frames, model3, m.l_alpha));
}

UIS_EXPORT int32_t uis_decode_device(uis_handle* h, const float* d_frames, const int64_t* offsets, int32_t n_utt,
                                     const uis_decode_opts* opts, int32_t* d_labels_out, float* d_scores_out,
                                     uis_stats* stats) {
  if (int rc = begin_call(h, "uis_decode_device", UIS_RULE_DECODE)) return rc;
  if (h) h->poison = UisPoison::from_env();
  return decode_impl(h, d_frames, offsets, n_utt, opts, d_labels_out, d_scores_out, stats);
}

// ------------------------------------------------------------------ device tensors in
#include "uis_ingest.hip"

UIS_EXPORT int32_t uis_ingest_tensors(uis_handle* h, const uis_tensor* blocks, int32_t n, void* producer_stream,
                                      float* d_frames_out, int64_t capacity_rows) {
  if (!h) return fail(UIS_ERR_INVALID_ARG, "null handle");
  int64_t F = 0;
  if (int rc = ingest_validate("uis_ingest_tensors", blocks, n, h->m.D, &F)) return rc;
  if (F > capacity_rows) return fail(UIS_ERR_INVALID_ARG, "uis_ingest_tensors: " + std::to_string((long long)F) + " rows given, capacity_rows is " + std::to_string((long long)capacity_rows));
  if (F > 0 && !d_frames_out) return fail(UIS_ERR_INVALID_ARG, "uis_ingest_tensors: d_frames_out is null");
  HIPCHK(hipSetDevice(h->device));
  if (int rc = ingest_enqueue(h, blocks, n, F, producer_stream, d_frames_out, UisPoison::from_env())) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  return UIS_OK;
}

UIS_EXPORT int32_t uis_tensors_decode(uis_handle* h, const uis_tensor* utterances, int32_t n_utt, void* producer_stream,
                                      const uis_decode_opts* opts, int32_t* d_labels_out, float* d_scores_out,
                                      uis_stats* stats) {
  static const char who[] = "uis_tensors_decode";
  if (int rc = begin_call(h, who, UIS_RULE_DECODE)) return rc;  // (the rule of every decode)
  if (!h) return fail(UIS_ERR_INVALID_ARG, "null handle");
  h->nb_valid = false;  // (as uis_decode: a decode refused below leaves nothing for uis_last_decode_nbest)
  h->last_U = 0; h->last_B = 0;
  int64_t F = 0;
  if (int rc = ingest_validate(who, utterances, n_utt, h->m.D, &F)) return rc;
  if (!opts) return fail(UIS_ERR_INVALID_ARG, "null opts");
  if (h->stream_state.active) return fail(UIS_ERR_INVALID_ARG, "a streaming session is open on this handle (uis_stream_end first)");
  std::vector<int64_t> offsets((size_t)n_utt + 1, 0);
  for (int u = 0; u < n_utt; ++u) offsets[u + 1] = offsets[u] + utterances[u].rows;
  HIPCHK(hipSetDevice(h->device));
  if (int rc = h->io_frames.ensure((size_t)std::max<int64_t>(F, 1) * h->m.D * 4)) return rc;
  h->poison = UisPoison::from_env();
  HIPCHK(h->poison.device(h->io_frames.p, h->io_frames.cap, h->stream));
  h->io_offsets.clear();  // (the labels go to the caller's tensor: nothing for uis_eval_last_decode)
  // the gather runs on the handle's stream, where the decode's first kernels follow it
  if (int rc = ingest_enqueue(h, utterances, n_utt, F, producer_stream, h->io_frames.as<float>(), h->poison)) return rc;
  const int rc = decode_impl(h, h->io_frames.as<float>(), offsets.data(), n_utt, opts, d_labels_out, d_scores_out, stats);
  // (a decode refused for its arguments has not waited for the gather: the caller's tensors are free on return)
  if (rc != UIS_OK && rc != UIS_ERR_CLUSTER_CAP) (void)hipStreamSynchronize(h->stream);
  return rc;
}

UIS_EXPORT int32_t uis_decode(uis_handle* h, const float* frames, const int64_t* offsets, int32_t n_utt,
                              const uis_decode_opts* opts, int32_t* labels_out, float* scores_out, uis_stats* stats) {
  if (h && !h->src64)  // (uis_decode_f64 has begun the call)
    if (int rc = begin_call(h, "uis_decode", UIS_RULE_DECODE)) return rc;
  if (!h || !offsets || n_utt < 0) return fail(UIS_ERR_INVALID_ARG, "null handle/offsets or negative n_utt");
  h->nb_valid = false;  // (a decode refused below leaves nothing for uis_last_decode_nbest either)
  const int64_t F = n_utt ? offsets[n_utt] : 0;
  if (F < 0) return fail(UIS_ERR_INVALID_ARG, "offsets must be non-decreasing");
  if (F > 0 && (!frames || !labels_out)) return fail(UIS_ERR_INVALID_ARG, "frames/labels_out is null");
  HIPCHK(hipSetDevice(h->device));
  int rc;
  if ((rc = h->io_frames.ensure((size_t)std::max<int64_t>(F, 1) * h->m.D * 4))) return rc;
  if ((rc = h->io_labels.ensure((size_t)std::max<int64_t>(F, 1) * 4))) return rc;
  if ((rc = h->io_scores.ensure((size_t)std::max(n_utt, 1) * 4))) return rc;
  if (!h->src64) h->poison = UisPoison::from_env();  // (uis_decode_f64 has read it)
  const UisPoison poison = h->poison;
  if (poison.on) {  // (the frames travel on the copy stream, behind ev_begin: uis_poison.h)
    HIPCHK(poison.device(h->io_frames.p, h->io_frames.cap, h->stream));
    HIPCHK(poison.device(h->io_labels.p, h->io_labels.cap, h->stream));
    HIPCHK(poison.device(h->io_scores.p, h->io_scores.cap, h->stream));
  }
  h->io_offsets.clear();
  rc = decode_impl(h, h->io_frames.as<float>(), offsets, n_utt, opts, h->io_labels.as<int32_t>(),
                   h->io_scores.as<float>(), stats, frames);
  if (rc != UIS_OK && rc != UIS_ERR_CLUSTER_CAP) return rc;
  if (rc == UIS_OK) h->io_offsets.assign(offsets, offsets + n_utt + 1);
  // uis_decode_f64 (the caller's label array is ordinary pageable memory, a numpy array): the labels
  // come down into a pinned block and are copied out by the CPU -- a device-to-pageable copy is staged
  // by the runtime in small pieces
  int32_t* lab_dst = labels_out;
  float* sc_dst = scores_out;
  if (h->src64) {
    const size_t need = (size_t)std::max<int64_t>(F, 1) * 4 + (size_t)std::max(n_utt, 1) * 4;
    if (h->h_out.ensure(need, hipHostMallocDefault) != hipSuccess) (void)hipGetLastError();  // (no pinned memory to be had: straight into the caller's arrays)
    poison.host(h->h_out.p, h->h_out.cap);  // (before the copies that land in it are enqueued)
    if (h->h_out.p) {
      lab_dst = h->h_out.as<int32_t>();
      sc_dst = reinterpret_cast<float*>(h->h_out.as<char>() + (size_t)std::max<int64_t>(F, 1) * 4);
    }
  }
  // (a copy that fails below fails the decode: then there is nothing for uis_last_decode_nbest either)
  struct NbestGuard {
    uis_handle* h; bool ok = false;
    ~NbestGuard() { if (!ok) h->nb_valid = false; }
  } nbest_guard{h};
  if (F > 0) HIPCHK(hipMemcpyAsync(lab_dst, h->io_labels.p, (size_t)F * 4, hipMemcpyDeviceToHost, h->stream));
  if (scores_out && n_utt > 0)
    HIPCHK(hipMemcpyAsync(sc_dst, h->io_scores.p, (size_t)n_utt * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  nbest_guard.ok = true;
  if (lab_dst != labels_out) {
    if (F > 0) memcpy(labels_out, lab_dst, (size_t)F * 4);
    if (scores_out && n_utt > 0) memcpy(scores_out, sc_dst, (size_t)n_utt * 4);
  }
  return rc;
}

UIS_EXPORT int32_t uis_decode_f64(uis_handle* h, const double* const* utterances, const int64_t* n_frames, int32_t n_utt,
                                  const uis_decode_opts* opts, int32_t* labels_out, float* scores_out, uis_stats* stats) {
  if (int rc = begin_call(h, "uis_decode_f64", UIS_RULE_DECODE)) return rc;
  if (!h || n_utt < 0 || (n_utt > 0 && (!utterances || !n_frames)))
    return fail(UIS_ERR_INVALID_ARG, "null handle/utterances/n_frames or negative n_utt");
  h->nb_valid = false;  // (as uis_decode: a decode refused below leaves nothing for uis_last_decode_nbest)
  std::vector<int64_t> offsets((size_t)n_utt + 1, 0);
  for (int u = 0; u < n_utt; ++u) {
    if (n_frames[u] < 0 || (n_frames[u] > 0 && !utterances[u])) return fail(UIS_ERR_INVALID_ARG, "negative n_frames or null utterance");
    offsets[u + 1] = offsets[u] + n_frames[u];
  }
  const int64_t F = offsets[n_utt];
  const size_t need = (size_t)std::max<int64_t>(F, 1) * h->m.D * 4;
  HIPCHK(hipSetDevice(h->device));
  const hipError_t e = h->h_cast.ensure(need, hipHostMallocDefault);  // grow only, like the device workspace
  if (e != hipSuccess) return fail(UIS_ERR_OOM, std::string("hipHostMalloc (float32 staging): ") + hipGetErrorString(e));
  h->poison = UisPoison::from_env();
  h->poison.host(h->h_cast.p, h->h_cast.cap);  // (before the cast team is posted)
  h->src64 = utterances;
  const int rc = uis_decode(h, h->h_cast.as<float>(), offsets.data(), n_utt, opts, labels_out, scores_out, stats);
  h->src64 = nullptr;
  return rc;
}

UIS_EXPORT int32_t uis_model_constants(uis_handle* h, float* m0_out, float* h1_out) {
  if (!h) return fail(UIS_ERR_INVALID_ARG, "null handle");
  const DevModel& m = h->m;
  HIPCHK(hipSetDevice(h->device));
  if (m0_out) {
    std::vector<float> tmp(m.Dp);
    HIPCHK(hipMemcpy(tmp.data(), m.m0, (size_t)m.Dp * 4, hipMemcpyDeviceToHost));
    memcpy(m0_out, tmp.data(), (size_t)m.D * 4);
  }
  if (h1_out) {
    std::vector<float> tmp((size_t)m.depth * m.Hp);
    HIPCHK(hipMemcpy(tmp.data(), m.h1, tmp.size() * 4, hipMemcpyDeviceToHost));
    const HidMap hmap{h->hid_map_seg, h->hid_map_seg_p};
    for (int l = 0; l < m.depth; ++l)
      for (int j = 0; j < h->H_model; ++j) h1_out[(size_t)l * h->H_model + j] = tmp[(size_t)l * m.Hp + hmap(j)];
  }
  return UIS_OK;
}

UIS_EXPORT int32_t uis_rnn_step(uis_handle* h, const float* x, const float* h_in, float* mean_out, float* h_out) {
  if (!h || !x || !h_in || !mean_out || !h_out) return fail(UIS_ERR_INVALID_ARG, "null argument");
  const DevModel& m = h->m;
  HIPCHK(hipSetDevice(h->device));
  const size_t hid_elems = (size_t)m.depth * m.Hp;
  std::vector<float> xp(m.Dp, 0.0f), hp(hid_elems, 0.0f), mo(m.Dp), ho(hid_elems);
  memcpy(xp.data(), x, (size_t)m.D * 4);
  const HidMap hmap{h->hid_map_seg, h->hid_map_seg_p};
  for (int l = 0; l < m.depth; ++l)
    for (int j = 0; j < h->H_model; ++j) hp[(size_t)l * m.Hp + hmap(j)] = h_in[(size_t)l * h->H_model + j];
  float *d_x = nullptr, *d_h = nullptr, *d_m = nullptr, *d_o = nullptr;
  Scratch tmp;
  int rc;
  if ((rc = tmp.get(&d_x, xp.size())) || (rc = tmp.get(&d_h, hp.size())) || (rc = tmp.get(&d_m, mo.size())) ||
      (rc = tmp.get(&d_o, ho.size())))
    return rc;
  HIPCHK(hipMemcpy(d_x, xp.data(), xp.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_h, hp.data(), hp.size() * 4, hipMemcpyHostToDevice));
  if ((rc = rnn_step_once(h, d_x, d_h, d_m, d_o))) return rc;
  HIPCHK(hipMemcpy(mo.data(), d_m, mo.size() * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(ho.data(), d_o, ho.size() * 4, hipMemcpyDeviceToHost));
  memcpy(mean_out, mo.data(), (size_t)m.D * 4);
  for (int l = 0; l < m.depth; ++l)
    for (int j = 0; j < h->H_model; ++j) h_out[(size_t)l * h->H_model + j] = ho[(size_t)l * m.Hp + hmap(j)];
  return UIS_OK;
}

UIS_EXPORT int32_t uis_last_decode_shape(uis_handle* h, int32_t* n_utt_out, int32_t* beam_size_out) {
  if (!h) return fail(UIS_ERR_INVALID_ARG, "null handle");
  if (n_utt_out) *n_utt_out = h->last_U;
  if (beam_size_out) *beam_size_out = h->last_B;
  return UIS_OK;
}

UIS_EXPORT int32_t uis_last_decode_info(uis_handle* h, int32_t* overflow_out, float* beam_scores_out) {
  if (!h) return fail(UIS_ERR_INVALID_ARG, "null handle");
  if (overflow_out && h->last_U) memcpy(overflow_out, h->last_overflow.data(), (size_t)h->last_U * 4);
  if (beam_scores_out && h->last_U) memcpy(beam_scores_out, h->last_beam_scores.data(), (size_t)h->last_U * h->last_B * 4);
  return UIS_OK;
}

UIS_EXPORT int32_t uis_last_decode_instantiation(uis_handle* h, int32_t out[5]) {
  if (!h || !out) return fail(UIS_ERR_INVALID_ARG, "null argument");
  const KernelPick& p = h->last_pick;
  out[0] = p.family; out[1] = p.Hp; out[2] = p.Dp; out[3] = p.variant; out[4] = p.persist;
  return UIS_OK;
}

UIS_EXPORT int32_t uis_decode_kernel_table(int32_t* rows, int32_t cap) {
  int32_t n = 0;
  for_each_kernel_table([&](const auto& table, int family, int persist) {
    for (const auto& e : table) {
      if (rows && n < cap) {
        int32_t* r = rows + (size_t)5 * n;
        r[0] = family; r[1] = e.Hp; r[2] = e.Dp; r[3] = e.variant; r[4] = persist;
      }
      ++n;
    }
  });
  return n;
}

UIS_EXPORT int32_t uis_debug_scores(uis_handle* h, float* scores_out, int64_t capacity) {
  if (!h || !scores_out) return fail(UIS_ERR_INVALID_ARG, "null argument");
  if (!h->dbg_floats) return fail(UIS_ERR_INVALID_ARG, "the last decode kept no candidate scores (UIS_FLAG_DEBUG_SCORES)");
  if (capacity < (int64_t)h->dbg_floats)
    return fail(UIS_ERR_INVALID_ARG, "uis_debug_scores: " + std::to_string((long long)h->dbg_floats) + " floats needed");
  if (hipSetDevice(h->device) != hipSuccess) return fail(UIS_ERR_HIP, "hipSetDevice");
  HIPCHK(hipMemcpy(scores_out, h->dbg_scores.p, h->dbg_floats * 4, hipMemcpyDeviceToHost));
  return UIS_OK;
}

// ------------------------------------------------------------------ streaming sessions
#include "uis_beam_view.h"
#include "uis_stream.hip"


// ------------------------------------------------------------------ evaluation
//
// Sequence-match accuracy on the device (uis_eval.hip): the step after predict() in the
// reference's demo (demo.py:61-66, uisrnn/evals.py:40-73).

namespace {

int eval_run(uis_handle* h, const int32_t* d_a, const int32_t* d_b, const int64_t* offsets, int32_t n_utt,
             int64_t* matched_out, const UisPoison& poison) {
  if (n_utt == 0) return UIS_OK;
  if (offsets[0] != 0) return fail(UIS_ERR_INVALID_ARG, "offsets[0] must be 0");
  for (int u = 0; u < n_utt; ++u)
    if (offsets[u + 1] < offsets[u]) return fail(UIS_ERR_INVALID_ARG, "offsets must be non-decreasing");
  int rc;
  if ((rc = h->ev_off.ensure((size_t)(n_utt + 1) * 8))) return rc;
  if ((rc = h->ev_out.ensure((size_t)n_utt * 12))) return rc;
  HIPCHK(poison.device(h->ev_off.p, h->ev_off.cap, h->stream));  // (UIS_POISON_WORKSPACE, as the entry point read it)
  HIPCHK(poison.device(h->ev_out.p, h->ev_out.cap, h->stream));
  long long* d_matched = h->ev_out.as<long long>();
  int32_t* d_status = reinterpret_cast<int32_t*>(d_matched + n_utt);
  HIPCHK(hipMemcpyAsync(h->ev_off.p, offsets, (size_t)(n_utt + 1) * 8, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_eval, dim3(n_utt), dim3(256), 0, h->stream, d_a, d_b, h->ev_off.as<int64_t>(), n_utt, d_matched,
                     d_status);
  HIPCHK(hipGetLastError());
  std::vector<int32_t> status(n_utt);
  static_assert(sizeof(long long) == sizeof(int64_t), "matched counts");
  HIPCHK(hipMemcpyAsync(matched_out, d_matched, (size_t)n_utt * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(status.data(), d_status, (size_t)n_utt * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int u = 0; u < n_utt; ++u) {
    if (status[u] == 1)
      return fail(UIS_ERR_UNSUPPORTED, "utterance " + std::to_string(u) + ": labels must lie in [0, 65536)");
    if (status[u] == 2)
      return fail(UIS_ERR_UNSUPPORTED, "utterance " + std::to_string(u) + ": more than 64 distinct labels in a sequence");
  }
  return UIS_OK;
}

}  // namespace

UIS_EXPORT int32_t uis_eval_accuracy_device(uis_handle* h, const int32_t* d_labels_a, const int32_t* d_labels_b,
                                            const int64_t* offsets, int32_t n_utt, int64_t* matched_out) {
  if (!h || !offsets || n_utt < 0 || (n_utt > 0 && !matched_out)) return fail(UIS_ERR_INVALID_ARG, "null argument or negative n_utt");
  if (n_utt > 0 && offsets[n_utt] > 0 && (!d_labels_a || !d_labels_b)) return fail(UIS_ERR_INVALID_ARG, "label pointer is null");
  HIPCHK(hipSetDevice(h->device));
  return eval_run(h, d_labels_a, d_labels_b, offsets, n_utt, matched_out, UisPoison::from_env());
}

UIS_EXPORT int32_t uis_eval_accuracy(uis_handle* h, const int32_t* labels_a, const int32_t* labels_b,
                                     const int64_t* offsets, int32_t n_utt, int64_t* matched_out) {
  if (!h || !offsets || n_utt < 0 || (n_utt > 0 && !matched_out)) return fail(UIS_ERR_INVALID_ARG, "null argument or negative n_utt");
  const int64_t F = n_utt ? offsets[n_utt] : 0;
  if (F > 0 && (!labels_a || !labels_b)) return fail(UIS_ERR_INVALID_ARG, "label pointer is null");
  HIPCHK(hipSetDevice(h->device));
  int rc;
  if ((rc = h->ev_a.ensure((size_t)std::max<int64_t>(F, 1) * 4))) return rc;
  if ((rc = h->ev_b.ensure((size_t)std::max<int64_t>(F, 1) * 4))) return rc;
  const UisPoison poison = UisPoison::from_env();
  HIPCHK(poison.device(h->ev_a.p, h->ev_a.cap, h->stream));
  HIPCHK(poison.device(h->ev_b.p, h->ev_b.cap, h->stream));
  if (F > 0) {
    HIPCHK(hipMemcpyAsync(h->ev_a.p, labels_a, (size_t)F * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->ev_b.p, labels_b, (size_t)F * 4, hipMemcpyHostToDevice, h->stream));
  }
  return eval_run(h, h->ev_a.as<int32_t>(), h->ev_b.as<int32_t>(), offsets, n_utt, matched_out, poison);
}

UIS_EXPORT int32_t uis_eval_last_decode(uis_handle* h, const int32_t* truth, int32_t n_utt, int64_t* matched_out) {
  if (!h || n_utt < 0 || (n_utt > 0 && !matched_out)) return fail(UIS_ERR_INVALID_ARG, "null argument or negative n_utt");
  if (h->io_offsets.empty() || (int)h->io_offsets.size() != n_utt + 1)
    return fail(UIS_ERR_INVALID_ARG, "no completed uis_decode with this many utterances on this handle");
  const int64_t F = h->io_offsets[n_utt];
  if (F > 0 && !truth) return fail(UIS_ERR_INVALID_ARG, "truth is null");
  HIPCHK(hipSetDevice(h->device));
  int rc;
  if ((rc = h->ev_b.ensure((size_t)std::max<int64_t>(F, 1) * 4))) return rc;
  const UisPoison poison = UisPoison::from_env();
  HIPCHK(poison.device(h->ev_b.p, h->ev_b.cap, h->stream));  // (io_labels: the last decode's, carried)
  if (F > 0) HIPCHK(hipMemcpyAsync(h->ev_b.p, truth, (size_t)F * 4, hipMemcpyHostToDevice, h->stream));
  // the predicted labels of the last uis_decode never left HBM for this
  return eval_run(h, h->io_labels.as<int32_t>(), h->ev_b.as<int32_t>(), h->io_offsets.data(), n_utt, matched_out, poison);
}

// ------------------------------------------------------------------ pinned host memory
UIS_EXPORT int32_t uis_host_alloc(size_t bytes, void** out) {
  if (!out) return fail(UIS_ERR_INVALID_ARG, "null out");
  *out = nullptr;
  hipError_t e = hipHostMalloc(out, std::max<size_t>(bytes, 1), hipHostMallocDefault);
  if (e != hipSuccess) { *out = nullptr; return fail(UIS_ERR_OOM, std::string("hipHostMalloc: ") + hipGetErrorString(e)); }
  return UIS_OK;
}

UIS_EXPORT void uis_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

// ------------------------------------------------------------------ scoring a given labeling
#include "uis_score.hip"

// ------------------------------------------------------------------ priming a session with a labeled prefix
#include "uis_prime.hip"

// ------------------------------------------------------------------ n-best readout
#include "uis_nbest.hip"

// ------------------------------------------------------------------ posterior readout
#include "uis_posterior.hip"

// ------------------------------------------------------------------ committing a session's final labels
#include "uis_commit.hip"

// ------------------------------------------------------------------ ending utterances of a session, reusing their slots
#include "uis_restart.hip"

// ------------------------------------------------------------------ retiring clusters no live hypothesis can name
#include "uis_retire.hip"

// ------------------------------------------------------------------ exporting / importing one utterance of a session
#include "uis_migrate.hip"
