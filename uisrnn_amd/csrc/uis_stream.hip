// uis_stream.hip -- the streaming sessions of the C ABI (uis_stream_*), included by uis_decoder.hip.
//
// Online decoding (the caller side of the path -- UIS-RNN is an online model, the
// reference only offers offline predict()).  A session keeps the beam, the cluster-state pool
// and the back-pointers of n_utt utterances on the device; uis_stream_push() appends frames (any
// number per utterance, also none) and advances every utterance by the frames it received;
// uis_stream_labels() reads the best hypothesis' labels for everything received so far.
// Semantics = predict_single with test_iteration 1 (uisrnn.py:479-562): pushing an utterance
// in any chunking gives bit for bit the labels / scores of one uis_decode over the whole of it
// (tests/test_gpu_stream.py).  look_ahead 1.  A push of four or more steps runs as ONE launch of
// k_decode_resident where that kernel applies, shorter pushes on the launch-per-step kernels.

namespace {

// One table of the session's state: an allocation of its own (the persistent launch's fixed row ranges and the L2
// note in alloc_persistent are why a session's addresses are left alone: no arena here).
template <typename T>
int stream_alloc(uis_handle* h, T** out, size_t count, bool zero = false) {
  DevBuf b;
  const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  if (int rc = b.alloc(bytes)) return rc;
  void* const p = b.p;
  *out = static_cast<T*>(p);  // (T may be const: a table DecodeState's kernels only read)
  h->stream_state.allocs.push_back(std::move(b));
  HIPCHK(h->stream_state.poison.device(p, bytes, h->stream));  // (UIS_POISON_WORKSPACE: ahead of the block's defining writes)
  if (zero) HIPCHK(hipMemsetAsync(p, 0, bytes, h->stream));
  return UIS_OK;
}

// ---- the persistent launch of a UIS_FLAG_PERSISTENT session
//
// Mailbox protocol (pm_block, host-coherent pinned memory; uint32 view, one 64-byte line per item,
// uis_kernels.h UIS_PM_*_WORD): a doorbell line per cluster {sequence number, command | frames << 8,
// first row | rows << 16} whose sequence number the host writes LAST (release) and rank 0 of the
// cluster polls with one 16-byte read; the sequence number of the last command each cluster
// completed; a word per cluster that turns non-zero when the cluster has left the kernel.
// While the launch is on the device the host makes NO HIP call that could wait for the device:
// everything a command needs was allocated by uis_stream_begin.

double pm_now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

unsigned long long pm_idle_ticks() {
  double ms = 50.0;  // without a command for this long the launch ends by itself (the next push starts a new one)
  if (const char* e = getenv("UIS_PERSIST_IDLE_MS")) ms = atof(e);
  ms = std::min(std::max(ms, 0.05), 2000.0);
  return (unsigned long long)(ms * 1e5);  // s_memrealtime ticks of 10 ns
}

// The abort word of the one-launch kernels (DecodeState::cl_abort = d_ctl + 16): non-zero once an in-launch barrier gave
// up, after which the session's state is not trustworthy any more.  Read behind the launch on the handle's stream and
// waited for (a push: its one synchronisation), or by a blocking copy where the stream is known to be drained
// (pm_reap, which then also gives the launch that stays up for this handle); `where` completes the message.
int launch_aborted(uis_handle* h, bool behind_launch, const char* where) {
  uint32_t word = 0;
  if (behind_launch) {
    HIPCHK(hipMemcpyAsync(&word, h->stream_state.d_ctl + 16, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  } else {
    HIPCHK(hipMemcpy(&word, h->stream_state.d_ctl + 16, 4, hipMemcpyDeviceToHost));
  }
  if (!word) return UIS_OK;
  if (!behind_launch) { h->stream_state.persist = false; h->resident_off = true; }
  return fail(UIS_ERR_HIP, std::string("in-launch barrier failed ") + where + "; close the session (uis_stream_end) and reopen it with UIS_FLAG_STEPWISE");
}

// After the launch has ended (every cluster left, or an in-launch barrier gave up): look at the abort word.
int pm_reap(uis_handle* h) {
  uis_handle::Stream& ss = h->stream_state;
  // (a launch that is really stuck must not take the caller with it: poll with a deadline instead
  // of an unbounded hipStreamSynchronize; the kernel's own barrier time-out is ~1 s)
  {
    const double t0 = pm_now_s();
    hipError_t q;
    while ((q = hipStreamQuery(h->stream)) == hipErrorNotReady) {
      if (pm_now_s() - t0 > 15.0) {
        ss.persist = false;
        h->resident_off = true;
        return fail(UIS_ERR_HIP, "the persistent streaming launch does not leave the device (15 s); the handle's "
                                 "stream is unusable -- destroy the handle");
      }
      __builtin_ia32_pause();
    }
    if (q != hipSuccess) return fail(UIS_ERR_HIP, std::string("hipStreamQuery: ") + hipGetErrorString(q));
  }
  ss.pm_running = false;
  return launch_aborted(h, false, "inside the persistent streaming launch");
}

int pm_launch(uis_handle* h) {
  uis_handle::Stream& ss = h->stream_state;
  const DevModel& m = h->m;
  DecodeState st = ss.st;
  // the mailbox as the device sees it (the same address under unified addressing; asked for anyway)
  void* blk = nullptr;
  HIPCHK(hipHostGetDevicePointer(&blk, ss.pm_block.p, 0));
  const MailboxLayout& box = ss.mailbox;
  st.x = ss.chunk.x.as<float>();  // (no header in front: the tables travel through the mailbox)
  st.gi0 = ss.chunk.gi0.as<float>();
  st.mse0 = ss.chunk.mse0.as<float>();
  st.push_F = 0;
  PersistArgs& pa = ss.pm_args;
  pa.ctl = static_cast<uint32_t*>(blk);
  pa.foff = uis_block_at<int64_t>(blk, box.o_foff);
  pa.avail = uis_block_at<int32_t>(blk, box.o_avail);
  pa.lab_off = uis_block_at<int64_t>(blk, box.o_lab_off);
  pa.frames = uis_block_at<float>(blk, box.o_frames);
  pa.labels = uis_block_at<int32_t>(blk, box.o_labels);
  pa.scores = uis_block_at<float>(blk, box.o_scores);
  pa.beam_scores = uis_block_at<float>(blk, box.o_beam_scores);
  pa.overflow = uis_block_at<int32_t>(blk, box.o_overflow);
  pa.go = ss.d_go;
  pa.hdr = ss.d_hdr;
  pa.hdr_stride = box.hdr_stride;
  pa.idle_ticks = pm_idle_ticks();
  HIPCHK(hipMemcpyAsync(ss.d_pm_args, &pa, sizeof(pa), hipMemcpyHostToDevice, h->stream));
  st.pm = ss.d_pm_args;
  // avail / foff only have to be non-null here (the kernel points them at its cluster's copies)
  st.avail = reinterpret_cast<const int32_t*>(ss.d_hdr);
  st.foff = reinterpret_cast<const int64_t*>(ss.d_hdr);
  HIPCHK(hipMemsetAsync(ss.d_ctl, 0, ss.ctl_words * 4, h->stream));
  HIPCHK(hipMemsetAsync(ss.d_go, 0, (size_t)UIS_PM_MAX_CLUSTERS * 128, h->stream));
  HIPCHK(hipMemsetAsync(ss.st.nrows, 0, 8, h->stream));
  Launcher lch{h, h->stream, false};
  h->inlaunch_failed = false;
  if (int rc = launch_cluster_kernel(lch, find_kernel(kernels::persist, m.Hp, m.Dp, CLS_NONE, &h->last_pick), h->n_cu, st.ncl,
                                     one_launch_lds(resident_lds_bytes(m.Hp, m.Dp, ss.B, ss.Kmax, ss.S)), m, st))
    return rc;
  ss.pm_running = true;
  ss.pm_launches += 1;
  return UIS_OK;
}

// Issue one command and wait until every cluster has completed it.  A launch that is not on the
// device (never started, or left because it was idle) is started first when `may_launch`; a
// launch that left while the command was on its way is reaped and the command issued again to a
// new one -- harmless: a cluster that did take a push has nothing left to do for it.
// Returns UIS_OK, an error, or PM_NOT_TAKEN = not running and may_launch was false.
constexpr int PM_NOT_TAKEN = 1;  // (no error: the caller goes through ordinary launches)
int pm_command(uis_handle* h, uint32_t type, uint32_t frames, bool may_launch, const uint32_t* row0 = nullptr,
               const uint32_t* nrow = nullptr) {
  uis_handle::Stream& ss = h->stream_state;
  volatile uint32_t* ctl = pm_ctl(ss);
  const int ncl = ss.st.ncl;
  for (int attempt = 0; attempt < 3; ++attempt) {
    int rc;
    if (!ss.pm_running) {
      if (!may_launch) return PM_NOT_TAKEN;
      for (int i = 0; i < UIS_PM_CTL_WORDS; ++i) ctl[i] = 0;
      ss.pm_seq = 1;
      pm_ring(ss, 1, type, frames, row0, nrow);
      if ((rc = pm_launch(h))) return rc;
    } else {
      ss.pm_seq += 1;
      pm_ring(ss, ss.pm_seq, type, frames, row0, nrow);
    }
    const double t0 = pm_now_s();
    bool left = false;
    unsigned spins = 0;
    for (;;) {
      bool all = true;
      for (int c = 0; c < ncl; ++c) all = all && ctl[UIS_PM_DONE_WORD + 16 * c] == ss.pm_seq;
      if (all) return UIS_OK;
      for (int c = 0; c < ncl; ++c) left = left || ctl[UIS_PM_LEFT_WORD + 16 * c] != 0;
      if (left) break;
      if ((++spins & 4095u) == 0) {
        if (pm_now_s() - t0 > 10.0) break;
        // (a launch that ended without saying so -- an in-launch barrier gave up -- is noticed here)
        if ((spins & 0xffffu) == 0 && hipStreamQuery(h->stream) == hipSuccess) { left = true; break; }
      }
      __builtin_ia32_pause();
    }
    // a cluster left before (or instead of) completing the command: tell the others to leave too
    // (they complete this command first if they had not seen it yet), then look at what happened
    ss.pm_seq += 1;
    pm_ring(ss, ss.pm_seq, UIS_PM_QUIT, 0);
    if ((rc = pm_reap(h))) return rc;
    if (!left) return fail(UIS_ERR_HIP, "the persistent streaming launch did not answer within 10 s");
  }
  return fail(UIS_ERR_HIP, "the persistent streaming launch kept leaving before it took the command");
}

int pm_quit(uis_handle* h) {
  uis_handle::Stream& ss = h->stream_state;
  if (!ss.pm_running) return UIS_OK;
  ss.pm_seq += 1;
  pm_ring(ss, ss.pm_seq, UIS_PM_QUIT, 0);
  return pm_reap(h);
}

// ---- the scaffold of a session call between launches: uis_stream_{labels, nbest, posterior, prime, commit, restart,
// retire, committed, limits, bindings, export, import} and uis_session_{min_turn, turns} (the getters stop after
// step 1; a push has an order of its own, above struct Push).  THE ORDER, stated here once:
//   1. session_of and the call's own checks on the host: nothing of the session is touched, and a call refused here
//      (or one with nothing to do) costs a UIS_FLAG_PERSISTENT session nothing and touches no device;
//   2. session_enter: the resident launch leaves (pm_quit -- it occupies every CU and the tables are written between
//      launches only, which keeps the XCD-private-L2 hazard described in uis_stream_begin away; ss.persist stays set,
//      the next push starts a new launch); frames in the window = steps run, from the host's own count `have` (the
//      `avail` table of the last push may live in a chunk buffer this path did not fill);
//   3. session_buffers: one ScratchPlan laid out in the one grow-only buffer sc_session, the pinned landing block, and
//      their fills (UIS_POISON_WORKSPACE: ahead of the defining writes);
//   4. the kernels between CallTimer::begin / end, ONE download, ONE hipStreamSynchronize;
//   5. the host's bookkeeping (have / committed / win_score, nb_valid), the call's trace line.
// Every store of every kernel is an ordinary vector store.

// the null-argument and no-session refusals (false: refused, UIS_ERR_INVALID_ARG with its message is recorded)
bool session_of(uis_handle* h, bool args = true, const char* null_msg = "null handle") {
  if (!h || !args) return !fail(UIS_ERR_INVALID_ARG, null_msg);
  return h->stream_state.active || !fail(UIS_ERR_INVALID_ARG, "no streaming session (uis_stream_begin first)");
}

// [U + 1] prefix sums of the frames in the utterances' windows
std::vector<int64_t> window_offsets(const uis_handle::Stream& ss) {
  std::vector<int64_t> off(ss.U + 1, 0);
  for (int u = 0; u < ss.U; ++u) off[u + 1] = off[u] + ss.have[u];
  return off;
}

// `view`: the session's tables with avail = the window's frame counts (null: the first half only -- uis_stream_prime
// reads no window, uis_stream_restart's readout has an avail table of its own)
int session_enter(uis_handle* h, DecodeState* view) {
  uis_handle::Stream& ss = h->stream_state;
  HIPCHK(hipSetDevice(h->device));
  if (int rc = ss.pm_running ? pm_quit(h) : UIS_OK) return rc;
  if (!view) return UIS_OK;
  HIPCHK(hipMemcpyAsync(ss.d_have, ss.have.data(), (size_t)ss.U * 4, hipMemcpyHostToDevice, h->stream));
  *view = ss.st;
  view->avail = ss.d_have;
  return UIS_OK;
}

// offsets into one block, in the order taken
struct ScratchPlan {
  size_t total = 0;
  size_t take(size_t bytes, size_t align = 16) { const size_t o = (total + align - 1) & ~(align - 1); total = o + bytes; return o; }
};

// the plan's block in sc_session (-> base), `land` bytes of pinned landing block (0: the call downloads nothing
// into it; with head-room: calls of a session vary in size), and the fills of both and of the call's `other` buffers
int session_buffers(uis_handle* h, const ScratchPlan& plan, size_t land, char** base, std::initializer_list<DevBuf*> other = {},
                    UisPoison* poison_out = nullptr) {
  uis_handle::Stream& ss = h->stream_state;
  if (int rc = h->sc_session.ensure(plan.total)) return rc;
  *base = h->sc_session.as<char>();
  if (land > ss.h_land.cap) {
    hipError_t e = ss.h_land.ensure(land + land / 4 + 4096, hipHostMallocDefault);
    if (e != hipSuccess) return fail(UIS_ERR_OOM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
  }
  const UisPoison poison = UisPoison::from_env();
  HIPCHK(poison.device(h->sc_session.p, h->sc_session.cap, h->stream));
  for (DevBuf* b : other) HIPCHK(poison.device(b->p, b->cap, h->stream));
  if (land) poison.host(ss.h_land.p, ss.h_land.cap);
  if (poison_out) *poison_out = poison;
  return UIS_OK;
}

// wall time from the call's entry, device time between begin() and end() (0 for a call that launched nothing);
// env(): the knob of the call's one line on stderr, read per call (a test turns it on)
struct CallTimer {
  uis_handle* h;
  std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
  bool device_work = false;
  hipError_t begin() { device_work = true; return hipEventRecord(h->ev_begin, h->stream); }
  hipError_t end() { return hipEventRecord(h->ev_end, h->stream); }
  static bool env(const char* name) { const char* e = getenv(name); return e && atoi(e) != 0; }
  double device_ms() const { float ms = 0.0f; if (device_work) (void)hipEventElapsedTime(&ms, h->ev_begin, h->ev_end); return (double)ms; }
  double call_ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(); }
};

// A call that asks one kernel about the session and changes nothing (uis_stream_bindings, uis_session_turns), after
// its checks: enter, one output block of `bytes` in the scratch plan, launch(view, block) between the timer's begin /
// end, one download, one synchronisation, the copy to `out`, the trace line where the call's knob asks for it.
template <typename Launch>
int session_query(uis_handle* h, const char* who, const char* trace_knob, size_t bytes, void* out, Launch launch) {
  uis_handle::Stream& ss = h->stream_state;
  CallTimer timer{h};
  DecodeState stv;
  if (int rc = session_enter(h, &stv)) return rc;
  ScratchPlan plan;
  const size_t o_out = plan.take(bytes);
  char* base;
  if (int rc = session_buffers(h, plan, bytes, &base)) return rc;
  HIPCHK(timer.begin());
  launch(stv, reinterpret_cast<int32_t*>(base + o_out));
  HIPCHK(hipGetLastError());
  HIPCHK(timer.end());
  HIPCHK(hipMemcpyAsync(ss.h_land.p, base + o_out, bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  memcpy(out, ss.h_land.p, bytes);
  if (CallTimer::env(trace_knob))
    fprintf(stderr, "%s: utterances %d device_ms %.3f call_ms %.3f\n", who, ss.U, timer.device_ms(), timer.call_ms());
  return UIS_OK;
}

// The prior tables logblk / logden of a session that must reach further (uis_stream_commit, uis_stream_import): they
// are indexed by block counts and their sum, which go on growing with the stream.  reserve() BEFORE any scratch (an
// allocation that fails leaves the session as it was): longer tables where `entries` exceeds what the session has, at
// least twice the length; blk / den go into session_buffers' `other` list; upload() after it (upload_log_tables'
// arithmetic: the common prefix keeps its bits); swap() after the synchronisation: the session is pointed at them and
// the old ones are freed, the launches that read them are over.
struct PriorTableGrowth {
  DevBuf blk, den;
  std::vector<double> host;
  int64_t len = 0;  // 0: the session's tables are long enough
  int reserve(uis_handle* h, int64_t entries) {
    const uis_handle::Stream& ss = h->stream_state;
    if (entries <= ss.log_len) return UIS_OK;
    len = std::max<int64_t>(2 * ss.log_len, entries);
    if (int rc = blk.alloc((size_t)len * 8)) return rc;
    return den.alloc((size_t)len * 8);
  }
  int upload(uis_handle* h) { return len ? upload_log_tables(h->alpha, len, host, blk.p, den.p, h->stream) : UIS_OK; }
  void swap(uis_handle* h) {
    if (!len) return;
    uis_handle::Stream& ss = h->stream_state;
    for (DevBuf& b : ss.allocs)  // the tables the session was opened or last grown with
      if (b.p == (void*)ss.st.logblk || b.p == (void*)ss.st.logden) b.release();
    ss.st.logblk = blk.as<double>();
    ss.st.logden = den.as<double>();
    ss.allocs.push_back(std::move(blk));
    ss.allocs.push_back(std::move(den));
    ss.log_len = len;
  }
};

// an utterance whose window a commit emptied still has its one hypothesis and its score: what the readouts show of
// it.  counts: 1; rank 0 of its `stride` values: `first` (null: win_score[u]), the `rest` after it: INFINITY; stable: 0;
// each where the pointer is set
void emptied_windows(const uis_handle::Stream& ss, int32_t* counts, float* values, size_t stride, const float* first,
                     int rest = 0, int64_t* stable = nullptr) {
  for (int u = 0; u < ss.U; ++u) {
    if (!ss.window_emptied(u)) continue;
    if (counts) counts[u] = 1;
    if (values) values[(size_t)u * stride] = first ? *first : ss.win_score[u];
    for (int k = 1; values && k <= rest; ++k) values[(size_t)u * stride + k] = INFINITY;
    if (stable) stable[u] = 0;
  }
}

// the readouts' last download: every group's overflow words, utterance order (null: not wanted)
int download_overflow(uis_handle* h, const std::vector<uis_handle::NbestGroup>& groups, int U, std::vector<int32_t>* overflow) {
  if (!overflow) return UIS_OK;
  overflow->assign(U, 0);
  for (const uis_handle::NbestGroup& g : groups)
    if (g.st.U > 0)
      HIPCHK(hipMemcpyAsync(overflow->data() + g.u0, g.st.overflow, (size_t)g.st.U * 4, hipMemcpyDeviceToHost, h->stream));
  return UIS_OK;
}

// The common body of uis_stream_nbest / uis_stream_posterior after their checks: enter, the session as the one group,
// `run` (the readout and its emptied-window fix-up), the overflow words' verdict.
template <typename Run>
int session_readout(uis_handle* h, Run run) {
  uis_handle::Stream& ss = h->stream_state;
  std::vector<uis_handle::NbestGroup> groups(1);
  if (int rc = session_enter(h, &groups[0].st)) return rc;  // (u0 = 0)
  std::vector<int32_t> overflow;
  if (int rc = run(groups, &overflow)) return rc;
  return cluster_cap_status(count_cluster_cap(overflow), ss.Kmax);
}

}  // namespace

namespace {

// DecodeState::limit from the caller's table (0: no bound); `dev` must outlive the copy
int upload_session_limits(uis_handle* h, const std::vector<int32_t>& limits, std::vector<int32_t>& dev) {
  uis_handle::Stream& ss = h->stream_state;
  dev.assign((size_t)ss.U, INT32_MAX);
  for (int u = 0; u < ss.U && u < (int)limits.size(); ++u)
    if (limits[u] > 0) dev[u] = limits[u];
  HIPCHK(hipMemcpyAsync(ss.st.limit, dev.data(), (size_t)ss.U * 4, hipMemcpyHostToDevice, h->stream));
  return UIS_OK;
}

// uis_stream_begin's: a session that is not opened to the end is released (stream_free) on every failing return, behind
// the stream (no upload may still be reading the call's host vectors)
struct SessionGuard {
  uis_handle* h;
  bool opened = false;
  ~SessionGuard() { if (!opened) { (void)hipStreamSynchronize(h->stream); stream_free(h); } }
};

}  // namespace

UIS_EXPORT int32_t uis_stream_begin(uis_handle* h, int32_t n_utt, const uis_decode_opts* opts, int64_t max_frames) {
  if (int rc = begin_call(h, "uis_stream_begin", UIS_RULE_STREAM_BEGIN)) return rc;
  if (!h || !opts || n_utt < 1 || max_frames < 1) return fail(UIS_ERR_INVALID_ARG, "null handle/opts, n_utt < 1 or max_frames < 1");
  uis_handle::Stream& ss = h->stream_state;
  if (ss.active) return fail(UIS_ERR_INVALID_ARG, "a streaming session is already open on this handle");
  if (int rc = table_status(h->tables.check_limits("session", n_utt))) return rc;
  const DevModel& m = h->m;
  const int B = opts->beam_size;
  const int Kmax = opts->max_clusters > 0 ? opts->max_clusters : 16;
  if (B < 1 || B > 256) return fail(UIS_ERR_UNSUPPORTED, "beam_size must be in [1, 256]");
  if (opts->look_ahead != 1) return fail(UIS_ERR_UNSUPPORTED, "streaming needs look_ahead 1");
  if (opts->test_iteration != 1) return fail(UIS_ERR_UNSUPPORTED, "streaming is online decoding: test_iteration must be 1");
  if (Kmax > 4096) return fail(UIS_ERR_UNSUPPORTED, "max_clusters must be <= 4096");
  if (max_frames > 0x7fffff00LL) return fail(UIS_ERR_UNSUPPORTED, "max_frames too large");
  const int U = n_utt, S = B * Kmax + B;
  const SelectLds lds = select_lds_layout(m.Dp, B, Kmax, S);
  if (lds.total > 160 * 1024) return fail(UIS_ERR_UNSUPPORTED, "beam_size * max_clusters too large for the select kernel's LDS budget");
  const double bytes = (double)U * S * (m.Dp + (double)m.depth * m.Hp) * 4.0 + (double)U * max_frames * B * 4.0;
  if (bytes > 200e9) return fail(UIS_ERR_OOM, "streaming state would need " + std::to_string((long long)(bytes / 1e9)) + " GB");
  HIPCHK(hipSetDevice(h->device));
  ss = uis_handle::Stream{};
  ss.poison = UisPoison::from_env();
  ss.U = U; ss.B = B; ss.Kmax = Kmax; ss.S = S; ss.cap = max_frames;
  ss.have.assign(U, 0);
  ss.committed.assign(U, 0);
  ss.win_score.assign(U, 0.0f);
  ss.min_turn.assign(U, 0);
  ss.log_len = max_frames + 2;
  DecodeState& st = ss.st;
  st.U = U; st.B = B; st.Kmax = Kmax; st.S = S; st.L = 1; st.tau = 1; st.flags = opts->flags | (agent_flags_env() ? UIS_FLAG_AGENT_FLAGS : 0u);
  st.max_rows = U * B;
  // a push advances the session with ONE launch of the resident decode kernel where that kernel
  // applies (same conditions as uis_decode); UIS_FLAG_STEPWISE keeps the four kernels per step
  const ClusterGeometry geo = cluster_geometry(h->n_cu, U, B, 0, 1);  // (one group, no row slack)
  // (streams never ran the 128-wide kernel)
  ss.resident = m.Hp != 128 && !(opts->flags & (UIS_FLAG_STEPWISE | UIS_FLAG_GENERIC_SELECT)) && resident_fits(m, U, B, Kmax, S, geo);
  if ((opts->flags & UIS_FLAG_RESIDENT) && !ss.resident)
    { ss = uis_handle::Stream{}; return fail(UIS_ERR_UNSUPPORTED, "UIS_FLAG_RESIDENT: the one-launch decode does not apply to this session's shape"); }
  std::vector<int64_t> off(U + 1);
  std::vector<double> log_host;
  std::vector<int32_t> limit_dev;
  SessionGuard guard{h};
  // ---- the session's state: one allocation per table (stream_alloc), ss.st pointed at them
  const StateCounts n = state_counts(m, U, B, Kmax, S, geo.rows_cap, 1);  // (one group)
  int rc = UIS_OK;
  const auto take = [&](auto** ptr, size_t count, bool zero = false) { if (!rc) rc = stream_alloc(h, ptr, count, zero); };
  take(&st.off, U + 1);
  take(&st.utt_step, U);
  take(&st.overflow, U);
  take(&st.limit, U);
  take(&ss.d_min_turn, U, true);  // (uis_session_min_turn: no slot has a rule, and st.min_turn stays null)
  take(&st.avail, U, true);  // (until the first push through ordinary launches points both into its chunk)
  take(&ss.d_have, U, true);
  take(&st.foff, U, true);
  take(&ss.d_lab_off, U, true);
  st.lab_off = ss.d_lab_off;
  take(&st.logblk, (size_t)ss.log_len);
  take(&st.logden, (size_t)ss.log_len);
  take(&st.pool_mean, n.pool_mean);
  take(&st.pool_hid, n.pool_hid);
  take(&st.pool_cnt, n.pool_cnt);
  take(&st.beam_n, n.beam_n);
  take(&st.beam_K, n.beam);
  take(&st.beam_last, n.beam);
  take(&st.beam_sum, n.beam);
  take(&st.beam_score, n.beam);
  take(&st.beam_slot, n.beam_lists);
  take(&st.beam_blk, n.beam_lists);
  // (a record per frame of the session's capacity; a decode's: per step of the frames given.  The table starts as zeros
  // -- under UIS_POISON_WORKSPACE as the poison word: the record word of a dead rank is never written, and
  // uis_stream_export copies the records verbatim, so without a defined start two sessions with the same history could
  // export different bytes)
  take(&st.bp, (size_t)U * max_frames * B, !ss.poison.on);
  take(&st.rows, n.rows, true);
  take(&st.nrows, n.nrows, true);
  take(&st.gi_up, n.gi_up);
  take(&st.a1, n.a1, true);
  take(&st.counters, 96, true);  // (one group's statistics words and room to spare; a decode's: every group's plus the diagnostic builds' clocks)
  ss.ctl_words = n.ctl_words;
  take(&ss.d_ctl, ss.ctl_words, true);
  take(&ss.d_beam_scores, (size_t)U * B);
  if (rc) return rc;
  wire_cluster_ctl(st, ss.d_ctl, ss.resident ? &geo : nullptr);
  if (opts->flags & UIS_FLAG_PERSISTENT) {
    // ---- the launch that stays: needs the one-launch shape with the beam in LDS (at most one utterance
    // per workgroup), unpadded frames, and a mailbox that holds every label of the session
    const bool shape = find_kernel(kernels::persist, m.Hp, m.Dp, CLS_NONE) != nullptr;
    const double label_bytes = (double)U * (double)max_frames * 4.0;
    if (!(ss.resident && shape && U <= 32 * geo.ncl && m.D == m.Dp && label_bytes <= 256e6))
      return fail(UIS_ERR_UNSUPPORTED, "UIS_FLAG_PERSISTENT needs the one-launch shape (rnn_depth 1, rnn_hidden_size 512 with "
                                       "observation_dim 256 / 512 or 256 with 256, unpadded), at most one utterance per compute "
                                       "unit and n_utt * max_frames <= 64 M labels");
    // Every cluster gets a FIXED row range of the chunk buffers (x, gi0, mse0) and of the mailbox's frame area
    // (MailboxLayout::cluster_rows).  Fixed, because the launch never ends between pushes: a row that changed hands from
    // one push to the next would leave a stale dirty line in the previous owner's XCD-private L2, free to be written back
    // over the new owner's data at any time (seen as rare score differences before the ranges were fixed).
    const MailboxLayout& box = ss.mailbox = MailboxLayout(U, B, m.D, max_frames, geo.ncl, UIS_PM_CTL_WORDS, UIS_RES_HEAD_TILES * 16 * 6);
    hipError_t e = ss.pm_block.ensure(box.total, hipHostMallocMapped | hipHostMallocCoherent);
    if (e != hipSuccess) return fail(UIS_ERR_OOM, std::string("hipHostMalloc (mailbox): ") + hipGetErrorString(e));
    ss.poison.host(ss.pm_block.p, box.total);  // (... and then the mailbox's initial state)
    memset(ss.pm_block.p, 0, box.total);
    take(&ss.d_go, (size_t)UIS_PM_MAX_CLUSTERS * 16, true);
    take(&ss.d_hdr, (size_t)geo.ncl * box.hdr_stride, true);
    take(&ss.d_pm_args, 1);
    // everything a push through the mailbox touches, now: no allocation while the launch is resident
    if (rc || (rc = ss.chunk.ensure(ChunkLayout(U, box.cap_frames, m.D, false, 0), box.cap_frames, m, false, false, false))) return rc;
    HIPCHK(ss.chunk.poison(ss.poison, h->stream));
    ss.persist = true;
  }
  // ---- the initial uploads
  if (ss.resident)  // the extra slot every GRU source row of a fresh cluster reads
    HIPCHK(hipMemcpyAsync(st.pool_hid + (size_t)U * S * m.Hp, m.h1, (size_t)m.Hp * 4, hipMemcpyDeviceToDevice, h->stream));
  for (int u = 0; u <= U; ++u) off[u] = (int64_t)u * max_frames;  // capacity offsets: they address the back-pointers
  // (the host fills three of the tables that the kernels, and so DecodeState, only read)
  HIPCHK(hipMemcpyAsync(const_cast<int64_t*>(st.off), off.data(), off.size() * 8, hipMemcpyHostToDevice, h->stream));
  ss.limits.assign((size_t)U, 0);
  if (h->tables.limits.call_set) ss.limits = h->tables.limits.call;
  if ((rc = upload_log_tables(h->alpha, ss.log_len, log_host, const_cast<double*>(st.logblk), const_cast<double*>(st.logden), h->stream))) return rc;
  hipLaunchKernelGGL(k_init_state, dim3((U + 255) / 256), dim3(256), 0, h->stream, st);
  HIPCHK(hipGetLastError());
  if ((rc = upload_session_limits(h, ss.limits, limit_dev))) return rc;  // (behind k_init_state, which has written "no bound")
  HIPCHK(hipStreamSynchronize(h->stream));  // (the host vectors go out of scope)
  ss.active = guard.opened = true;
  return UIS_OK;
}

namespace {

// ---- a push (uis_stream_push, uis_tensors_stream_push).  THE ORDER, stated here once (the steps of struct Push):
//   1. checks, on the host: the counts against the window's capacity and the 2^31 - 256 bound, this push's tables,
//      what a UIS_FLAG_PERSISTENT session cannot take, the 2^24 bound of a tagged session.  Nothing of the session is
//      touched; a push that brings no frame ends here;
//   2. through_mailbox: a persistent session whose clusters' shares fit their fixed row ranges -- tables and frames
//      into the mailbox, ring, wait.  No HIP call unless the launch has to be started.  Every other push goes on:
//   3. upload: a resident launch leaves; the chunk's layout, its growth and fills, the bias and tag tables, the
//      staging block and its ONE H2D, the gather for tensors, the pad kernel;
//   4. launch: stepwise / one launch / fused, the cooperative launch and its refusal's fallback, enqueue_steps;
//   5. in run(): the ONE hipStreamSynchronize, behind a one-launch kernel with the abort word and its
//      verdict (launch_aborted); and the bookkeeping (have), once for both ways.
// Who brings the frames: `frames` (uis_stream_push: host float32, utterance after utterance) or `chunks`
// (uis_tensors_stream_push: one device tensor per utterance, gathered by k_ingest into the chunk's frame area) -- exactly
// one of the two is given.  The caller has begun the call and checked the handle and the session.
struct Push {
  uis_handle* const h;
  const char* who;
  const float* frames;
  const uis_tensor* chunks;
  void* producer_stream;
  const int32_t* counts;
  uis_handle::Stream& ss = h->stream_state;
  int64_t F = 0, max_new = 0;  // (1) the frames of the push; the most any utterance brings = the steps to run
  const float* d_x = nullptr;  // (3) the chunk's frames as the kernels read them (padded where D != Dp)
  bool ran_resident = false;   // (4) a one-launch kernel took the push

  int checks() {
    for (int u = 0; u < ss.U; ++u) {
      if (counts[u] < 0) return fail(UIS_ERR_INVALID_ARG, "negative frame count");
      if ((int64_t)ss.have[u] + counts[u] > ss.cap)
        return fail(UIS_ERR_INVALID_ARG, "utterance exceeds the session's max_frames (the window of frames not yet committed: "
                                         "uis_stream_commit makes room)");
      // (pool_cnt / beam_sum count everything an utterance ever received, in int32)
      if (ss.committed[u] + ss.have[u] + counts[u] > 0x7fffff00LL)
        return fail(UIS_ERR_UNSUPPORTED, "utterance would have received more than 2^31 - 256 frames in this session");
      F += counts[u];
      max_new = std::max<int64_t>(max_new, counts[u]);
    }
    if (int rc = table_status(h->tables.check_bias("call", F))) return rc;
    // (the resident launch of a UIS_FLAG_PERSISTENT session reads its priors from the kernel arguments it was launched with;
    // a table would have to travel through the mailbox, whose layout is a protocol of its own: DESIGN.md section 9, "Open")
    if (h->tables.bias3.call_set && (ss.st.flags & UIS_FLAG_PERSISTENT))
      return fail(UIS_ERR_UNSUPPORTED, "a UIS_FLAG_PERSISTENT session takes no per-frame transition_bias (uis_frame_bias): the table is dropped");
    // (uis_stream_speakers: the same three checks for this push's tags, then the 2^24 bound of a session that holds any)
    if (int rc = table_status(h->tables.check_stream_tags("call", F))) return rc;
    if (h->tables.stream_tags.call_set && (ss.st.flags & UIS_FLAG_PERSISTENT))
      return fail(UIS_ERR_UNSUPPORTED, "a UIS_FLAG_PERSISTENT session takes no known speakers (uis_stream_speakers): the table is dropped");
    for (int u = 0; u < ss.U; ++u)
      if (int rc = table_status(CallTables::check_tagged_frames(who, ss.tagged || h->tables.tagged, u, ss.committed[u] + ss.have[u] + counts[u]))) return rc;
    return UIS_OK;
  }

  // The launch that stays on the device.  Returns UIS_OK: the push is done; an error; or PM_NOT_TAKEN: this push goes through
  // ordinary launches (no persistent session, tensors -- they never reach one --, a cluster's share that does not fit,
  // or the cooperative launch was refused: ordinary launches from here on).
  int through_mailbox() {
    const MailboxLayout& box = ss.mailbox;
    const int D = h->m.D, ncl = ss.st.ncl;
#if defined(UIS_PM_TIMING)
    const double t_enter = pm_now_s();
#endif
    if (!ss.persist || h->resident_off || chunks || !chunk_rows(ss.U, ncl, box.cluster_rows, counts, nullptr, nullptr, nullptr, nullptr, nullptr))
      return PM_NOT_TAKEN;
    // frames cluster by cluster: each cluster's rank 0 fetches ONE contiguous row range
    void* const pm = ss.pm_block.p;
    uint32_t row0[UIS_PM_MAX_CLUSTERS], nrow[UIS_PM_MAX_CLUSTERS];
    int64_t* foff = uis_block_at<int64_t>(pm, box.o_foff);
    chunk_rows(ss.U, ncl, box.cluster_rows, counts, ss.have.data(), foff, uis_block_at<int32_t>(pm, box.o_avail), row0, nrow);
    const float* src = frames;  // (utterance after utterance in the caller's buffer)
    for (int u = 0; u < ss.U; src += (size_t)counts[u] * D, ++u)
      if (counts[u]) memcpy(uis_block_at<float>(pm, box.o_frames) + (size_t)(foff[u] + ss.have[u]) * D, src, (size_t)counts[u] * D * 4);
    h->inlaunch_failed = false;
#if defined(UIS_PM_TIMING)
    static double fill_s = 0.0, wait_s = 0.0; static long n_push = 0;
    const double t_mid = pm_now_s();
    fill_s += t_mid - t_enter;
#endif
    const int rc = pm_command(h, UIS_PM_PUSH, (uint32_t)std::min<int64_t>(F, 4095), true, row0, nrow);
#if defined(UIS_PM_TIMING)
    wait_s += pm_now_s() - t_mid;
    if (++n_push % 100 == 0) {
      const volatile unsigned long long* k = reinterpret_cast<const volatile unsigned long long*>(pm_ctl(ss) + UIS_PM_TIMING_WORD);
      const unsigned long long k5 = k[5]; const double n = (double)(k5 ? k5 : 1);
      fprintf(stderr, "[pm timing] host per push: fill %.1f us, ring + wait %.1f us; kernel (workgroup 0) per push: fetch %.1f, pass on %.1f, "
              "count + chunk projection %.1f, steps %.1f us\n", 1e6 * fill_s / n_push, 1e6 * wait_s / n_push, k[0] * 0.01 / n, k[1] * 0.01 / n,
              k[2] * 0.01 / n, k[3] * 0.01 / n);
    }
#endif
    if (rc == UIS_OK || !h->inlaunch_failed) return rc;
    ss.persist = false;
    return PM_NOT_TAKEN;
  }

  int upload() {
    const bool with_bias = h->tables.bias3.call_set, with_tags = h->tables.stream_tags.call_set;
    int rc;
    if (ss.pm_running && (rc = pm_quit(h))) return rc;
    Chunk& ck = ss.chunk;
    const ChunkLayout lay(ss.U, F, h->m.D, chunks != nullptr, sizeof(IngestBlock));
    if ((rc = ck.ensure(lay, F, h->m, with_bias, with_tags))) return rc;
    // UIS_POISON_WORKSPACE: a push through ordinary launches rebuilds its chunk from nothing (the session's state lives
    // elsewhere) -- all on the handle's stream, idle since the last call
    ss.poison = UisPoison::from_env();
    if (ss.poison.on) HIPCHK(ck.poison(ss.poison, h->stream));
    // (the table's rows are the chunk's: row foff[u] + step, as mse0; the call's table lives until the synchronize below)
    if (with_bias) HIPCHK(hipMemcpyAsync(ck.bias.p, h->tables.bias3.data(), (size_t)F * 24, hipMemcpyHostToDevice, h->stream));
    // (the tags likewise, one byte per chunk row; the session counts as tagged from here on, whatever becomes of the push)
    if (with_tags) HIPCHK(hipMemcpyAsync(ck.hint.p, h->tables.stream_tags.data(), (size_t)F, hipMemcpyHostToDevice, h->stream));
    ss.tagged = ss.tagged || h->tables.tagged;
    // one staging block, one H2D; for tensors the frame area behind the header is written by the gather
    chunk_rows(ss.U, 1, 0, counts, ss.have.data(), uis_block_at<int64_t>(ck.stage.p, lay.o_foff), uis_block_at<int32_t>(ck.stage.p, lay.o_avail), nullptr, nullptr);
    float* const d_frames = uis_block_at<float>(ck.x.p, lay.o_frames);
    if (frames) memcpy(uis_block_at<float>(ck.stage.p, lay.o_frames), frames, (size_t)F * h->m.D * 4);
    else ingest_fill_table(ck.stage.as<IngestBlock>(), chunks, ss.U, h->m.D, d_frames);
    HIPCHK(hipMemcpyAsync(ck.x.p, ck.stage.p, lay.travel_bytes, hipMemcpyHostToDevice, h->stream));
    if (chunks && (rc = ingest_launch(h, ck.x.as<IngestBlock>(), ss.U, F, producer_stream, d_frames))) return rc;
    ss.st.foff = uis_block_at<int64_t>(ck.x.p, lay.o_foff);
    ss.st.avail = uis_block_at<int32_t>(ck.x.p, lay.o_avail);
    d_x = d_frames;
    if (h->m.D != h->m.Dp) {
      hipLaunchKernelGGL(k_pad_frames, dim3((unsigned)(((long)F * h->m.Dp + 255) / 256)), dim3(256), 0, h->stream, d_x, ck.pad.as<float>(), (long)F, h->m.D, h->m.Dp);
      HIPCHK(hipGetLastError());
      d_x = ck.pad.as<float>();
    }
    return UIS_OK;
  }

  int launch() {
    float *const gi0 = ss.chunk.gi0.as<float>(), *const mse0 = ss.chunk.mse0.as<float>();
    int rc;
    Launcher lch{h, h->stream, false};
    DecodeState st = ss.st;
    st.x = d_x; st.gi0 = gi0; st.mse0 = mse0;
    st.bias3 = h->tables.bias3.call_set ? ss.chunk.bias.as<double>() : nullptr;  // (ss.st.bias3 stays null: no other session call forms a prior)
    st.hint = h->tables.stream_tags.call_set ? ss.chunk.hint.as<uint8_t>() : nullptr;  // (ss.st.hint likewise: the bindings ride in beam_blk)
    // One-launch path: the chunk's projection fused into the kernel and plain launches after the
    // session's first push make a push one H2D, one memset and ONE kernel.  Measured
    // (tools/stream_latency.py, profiles/): that kernel re-reads its weights into registers / LDS at
    // every launch (~10 us), so for 1-3 steps per push the four small kernels per step are still
    // quicker (79 vs 96 us for one frame of 64 utterances); from 4 steps on the single launch wins
    // (16 frames: 690 vs 880 us).  UIS_FLAG_RESIDENT forces it, UIS_FLAG_STEPWISE forbids it.
    bool stepwise = !ss.resident || h->resident_off || (max_new < UIS_STREAM_RESIDENT_MIN_STEPS && !(ss.st.flags & UIS_FLAG_RESIDENT));
    // the chunk's gi0 / mse0: inside the one-launch kernel when the frames need no padding and the
    // chunk's rows fit the kernel's LDS list, else by the two once-per-chunk kernels
    const bool fused = !stepwise && h->m.D == h->m.Dp && F <= (int64_t)UIS_RES_HEAD_TILES * 16 * 6;
    if (!fused && (rc = plain_input_proj(lch, h->m, d_x, gi0, mse0, (long)F))) return rc;
    HIPCHK(hipMemsetAsync(ss.st.nrows, 0, 8, h->stream));
    st.push_F = fused ? (int)F : 0;
    if (!stepwise) {
      // every step of this push in ONE launch (the kernel runs max over utterances of
      // avail - utt_step steps; utterances without new frames sit them out)
      HIPCHK(hipMemsetAsync(ss.d_ctl, 0, ss.ctl_words * 4, h->stream));
      h->inlaunch_failed = false;
      // Every push is a COOPERATIVE launch: the kernel spins on in-launch barriers and needs all its
      // workgroups co-resident, which only that launch path checks against whatever else runs on the
      // device at that moment (another handle's decode, a second session).  A plain launch of the
      // same grid saves 15-19 us of host time per push; it is opt-in (UIS_STREAM_PLAIN_LAUNCH=1) for
      // callers that own the device, and used only after the session's first push went through the
      // cooperative path.
      static const bool plain_ok = getenv("UIS_STREAM_PLAIN_LAUNCH") != nullptr && atoi(getenv("UIS_STREAM_PLAIN_LAUNCH")) != 0;
      rc = launch_cluster_kernel(lch, find_kernel(kernels::resident, h->m.Hp, h->m.Dp, CLS_NONE, &h->last_pick), h->n_cu, st.ncl,
                                 one_launch_lds(resident_lds_bytes(h->m.Hp, h->m.Dp, ss.B, ss.Kmax, ss.S)), h->m, st,
                                 !(ss.coop_checked && plain_ok));
      if (rc && h->inlaunch_failed) {  // refused before anything ran: the per-step kernels take over
        h->resident_off = true; stepwise = true;
        if (fused) {  // ... and they need the chunk's gi0 / mse0
          if ((rc = plain_input_proj(lch, h->m, d_x, gi0, mse0, (long)F))) return rc;
          st.push_F = 0;
        }
      } else if (rc) return rc;
      else { ran_resident = true; ss.coop_checked = true; }
    }
    if (stepwise) {
      h->last_pick = KernelPick{};
      h->last_pick.family = UIS_DK_STEPWISE; h->last_pick.Hp = h->m.Hp; h->last_pick.Dp = h->m.Dp;
      if ((rc = enqueue_steps(h, lch, st, select_lds_layout(h->m.Dp, ss.B, ss.Kmax, ss.S).total, (int)max_new))) return rc;
    }
    return UIS_OK;
  }

  int run() {
    if (int rc = checks()) return rc;
    if (F == 0) return UIS_OK;
    if (!frames && !chunks) return fail(UIS_ERR_INVALID_ARG, "frames is null");
    HIPCHK(hipSetDevice(h->device));
    int rc = through_mailbox();
    if (rc == PM_NOT_TAKEN) {
      if ((rc = upload())) return rc;
      if ((rc = launch())) return rc;
      // (5: after the synchronisation the staging block and the caller's frames may be reused)
      if (ran_resident) rc = launch_aborted(h, true, "during uis_stream_push");
      else HIPCHK(hipStreamSynchronize(h->stream));
    }
    if (rc) return rc;
    for (int u = 0; u < ss.U; ++u) ss.have[u] += counts[u];
    return UIS_OK;
  }
};

}  // namespace

UIS_EXPORT int32_t uis_stream_push(uis_handle* h, const float* frames, const int32_t* counts) {
  if (int rc = begin_call(h, "uis_stream_push", UIS_RULE_STREAM_PUSH)) return rc;  // (this push's tables, in the chunk's own frame order)
  if (!session_of(h, counts != nullptr, "null handle/counts")) return UIS_ERR_INVALID_ARG;
  return Push{h, "uis_stream_push", frames, nullptr, nullptr, counts}.run();
}

UIS_EXPORT int32_t uis_tensors_stream_push(uis_handle* h, const uis_tensor* chunks, void* producer_stream) {
  static const char who[] = "uis_tensors_stream_push";
  if (int rc = begin_call(h, who, UIS_RULE_STREAM_PUSH)) return rc;  // (uis_stream_push's rule: this push's tables)
  if (!session_of(h, chunks != nullptr, "null handle/chunks")) return UIS_ERR_INVALID_ARG;
  uis_handle::Stream& ss = h->stream_state;
  // (the resident launch of a UIS_FLAG_PERSISTENT session takes its frames from the host mailbox)
  if (ss.st.flags & UIS_FLAG_PERSISTENT)
    return fail(UIS_ERR_UNSUPPORTED, "a UIS_FLAG_PERSISTENT session takes no device tensors (uis_tensors_stream_push): its frames travel "
                                     "through the host mailbox; use uis_stream_push");
  int64_t F = 0;
  if (int rc = ingest_validate(who, chunks, ss.U, h->m.D, &F)) return rc;
  std::vector<int32_t> counts((size_t)ss.U);
  for (int u = 0; u < ss.U; ++u) {
    if (chunks[u].rows > 0x7fffff00LL) return fail(UIS_ERR_INVALID_ARG, "utterance exceeds the session's max_frames");
    counts[u] = (int32_t)chunks[u].rows;
  }
  return Push{h, who, nullptr, chunks, producer_stream, counts.data()}.run();
}

UIS_EXPORT int32_t uis_stream_labels(uis_handle* h, int32_t* labels_out, float* scores_out, int32_t* overflow_out) {
  if (int rc = begin_call(h, "uis_stream_labels", UIS_RULE_STREAM_OTHER)) return rc;
  if (!session_of(h)) return UIS_ERR_INVALID_ARG;
  uis_handle::Stream& ss = h->stream_state;
  const int U = ss.U;
  const size_t nb = (size_t)U * ss.B;
  const std::vector<int64_t> lab_off = window_offsets(ss);
  const int64_t F = lab_off[U];
  if (F > 0 && !labels_out) return fail(UIS_ERR_INVALID_ARG, "labels_out is null");
  HIPCHK(hipSetDevice(h->device));
  int rc = PM_NOT_TAKEN;  // (no resident launch to ask)
  const MailboxLayout& box = ss.mailbox;
  void* const pm = ss.pm_block.p;
  if (ss.persist && ss.pm_running) {
    // the resident launch back-traces every utterance and writes into the mailbox
    memcpy(uis_block_at<int64_t>(pm, box.o_lab_off), lab_off.data(), (size_t)U * 8);
    rc = pm_command(h, UIS_PM_LABELS, 0, false);
    if (rc != UIS_OK && rc != PM_NOT_TAKEN) return rc;  // (not taken: the launch had left -- its tables are back in global memory)
  }
  if (rc == UIS_OK) {
    if (F > 0) memcpy(labels_out, uis_block_at<int32_t>(pm, box.o_labels), (size_t)F * 4);
    if (scores_out) memcpy(scores_out, uis_block_at<float>(pm, box.o_scores), (size_t)U * 4);
    h->last_overflow.assign(uis_block_at<int32_t>(pm, box.o_overflow), uis_block_at<int32_t>(pm, box.o_overflow) + U);
    h->last_beam_scores.assign(uis_block_at<float>(pm, box.o_beam_scores), uis_block_at<float>(pm, box.o_beam_scores) + nb);
  } else {
    DecodeState stl;
    if ((rc = session_enter(h, &stl))) return rc;  // (no launch is running here: the mailbox path above took it or found it gone)
    if ((rc = ss.labels.ensure((size_t)std::max<int64_t>(F, 1) * 4))) return rc;
    if ((rc = ss.scores.ensure((size_t)U * 4))) return rc;
    const UisPoison poison = UisPoison::from_env();
    HIPCHK(poison.device(ss.labels.p, ss.labels.cap, h->stream));
    HIPCHK(poison.device(ss.scores.p, ss.scores.cap, h->stream));
    HIPCHK(hipMemcpyAsync(ss.d_lab_off, lab_off.data(), (size_t)U * 8, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_backtrace, dim3(U), dim3(64), (size_t)64 * ss.B, h->stream, stl, ss.labels.as<int32_t>(),
                       ss.scores.as<float>(), ss.d_beam_scores);
    HIPCHK(hipGetLastError());
    if (F > 0) HIPCHK(hipMemcpyAsync(labels_out, ss.labels.p, (size_t)F * 4, hipMemcpyDeviceToHost, h->stream));
    if (scores_out) HIPCHK(hipMemcpyAsync(scores_out, ss.scores.p, (size_t)U * 4, hipMemcpyDeviceToHost, h->stream));
    h->last_overflow.assign(U, 0);
    h->last_beam_scores.assign(nb, INFINITY);
    HIPCHK(hipMemcpyAsync(h->last_overflow.data(), ss.st.overflow, (size_t)U * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(h->last_beam_scores.data(), ss.d_beam_scores, nb * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  // ---- the tail of both ways: the "last decode" of uis_last_decode_info / _shape is this session from here on (the
  // readout follows); what is shown of a window that a commit emptied; the overflow words' verdict
  h->last_U = U; h->last_B = ss.B;
  h->nb_valid = false;
  emptied_windows(ss, nullptr, scores_out, 1, nullptr);
  emptied_windows(ss, nullptr, h->last_beam_scores.data(), ss.B, nullptr, ss.B - 1);
  return cluster_cap_status(count_cluster_cap(h->last_overflow, overflow_out), ss.Kmax);
}

UIS_EXPORT int32_t uis_stream_end(uis_handle* h) {
  if (int rc = begin_call(h, "uis_stream_end", UIS_RULE_STREAM_OTHER)) return rc;
  if (!h) return fail(UIS_ERR_INVALID_ARG, "null handle");
  if (!h->stream_state.active) return UIS_OK;
  HIPCHK(hipSetDevice(h->device));
  const int rc_quit = pm_quit(h);
  HIPCHK(hipStreamSynchronize(h->stream));
  stream_free(h);
  return rc_quit;
}

// max_speakers of an open session.  The table belongs to the slots, not to the streams in them: restarts, imports and
// retirements leave it alone, blobs do not carry it.  All or nothing: a table with a value out of range changes none.
UIS_EXPORT int32_t uis_stream_limits(uis_handle* h, const int32_t* limits) {
  if (int rc = begin_call(h, "uis_stream_limits", UIS_RULE_STREAM_OTHER)) return rc;
  if (!session_of(h, limits != nullptr, "null handle/limits")) return UIS_ERR_INVALID_ARG;
  uis_handle::Stream& ss = h->stream_state;
  for (int u = 0; u < ss.U; ++u)
    if (limits[u] < 0 || limits[u] > 4096) return fail(UIS_ERR_INVALID_ARG, "a limit must be in [0, 4096] (0: no bound)");
  if (int rc = session_enter(h, nullptr)) return rc;  // (the resident launch leaves: the table is written between launches)
  const std::vector<int32_t> next(limits, limits + ss.U);
  std::vector<int32_t> dev;
  if (int rc = upload_session_limits(h, next, dev)) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  ss.limits = next;
  return UIS_OK;
}

namespace {

#define UIS_BINDINGS_WIDTH 128   // tags 0 .. 127: one thread and one output word each

// The binding of the best hypothesis, one workgroup per utterance, between launches: out[u][g] = the cluster index whose
// block-count word of rank 0 carries tag g (1 .. 127), -1 where none does; out[u][0] = how many tags are bound.  An
// utterance without a live hypothesis (an emptied beam, the overflow word set): 0 and -1 everywhere.  A window that a
// commit emptied keeps its one hypothesis, and with it the binding.
__global__ __launch_bounds__(UIS_BINDINGS_WIDTH) void k_stream_bindings(DecodeState st, int32_t* __restrict__ out) {
  __shared__ int s_bound[UIS_BINDINGS_WIDTH];
  const int u = blockIdx.x, tid = threadIdx.x;
  if (u >= st.U) return;
  const auto [N, T, par, nb, live, e, bp] = beam_view(st, u, EMPTY_WINDOW_KEEPS_BEAM);
  s_bound[tid] = -1;
  __syncthreads();
  if (live > 0) {
    int K = st.beam_K[e];
    K = K < 0 ? 0 : (K > st.Kmax ? st.Kmax : K);
    const int32_t* row = st.beam_blk + e * st.Kmax;   // rank 0
    for (int k = tid; k < K; k += UIS_BINDINGS_WIDTH) {
      const int g = blk_tag(row[k]) & (UIS_BINDINGS_WIDTH - 1);
      if (g) s_bound[g] = k;   // (a binding is injective: no two threads write one word)
    }
  }
  __syncthreads();
  const int c = s_bound[tid];
  const int n = __syncthreads_count(tid > 0 && c >= 0);
  out[(size_t)u * UIS_BINDINGS_WIDTH + tid] = tid == 0 ? n : c;
}

}  // namespace

// Who is who right now: see include/uisrnn_hip.h.  The scaffold's order; nothing of the session changes.
UIS_EXPORT int32_t uis_stream_bindings(uis_handle* h, int32_t* out) {
  if (int rc = begin_call(h, "uis_stream_bindings", UIS_RULE_STREAM_OTHER)) return rc;
  if (!session_of(h, out != nullptr, "null handle/out")) return UIS_ERR_INVALID_ARG;
  const int U = h->stream_state.U;
  return session_query(h, "uis_stream_bindings", "UIS_BINDINGS_TRACE", (size_t)U * UIS_BINDINGS_WIDTH * 4, out, [&](const DecodeState& stv, int32_t* d_out) {
    hipLaunchKernelGGL(k_stream_bindings, dim3(U), dim3(UIS_BINDINGS_WIDTH), 0, h->stream, stv, d_out);
  });
}

UIS_EXPORT int32_t uis_stream_get_limits(uis_handle* h, int32_t* out) {
  if (int rc = begin_call(h, "uis_stream_get_limits", UIS_RULE_STREAM_OTHER)) return rc;
  if (!session_of(h, out != nullptr, "null handle/out")) return UIS_ERR_INVALID_ARG;
  const uis_handle::Stream& ss = h->stream_state;
  for (int u = 0; u < ss.U; ++u) out[u] = ss.limits[u];
  return UIS_OK;
}

// ---- the minimum turn length of an open session's slots.  The table belongs to the slots, as
// max_speakers does: restarts keep it, blobs do not carry it, an imported utterance decodes on under the target slot's
// value.  The run rides in the last-label words the session already keeps (uis_kernels.h UIS_LAST_*); the selects of
// every push read utt_min_turn(st, u), so a push needs nothing but DecodeState::min_turn -- set exactly while some slot
// has a value of 2 or more: a session without a rule hands its kernels a null pointer, as before.

namespace {

// the opener of the uis_session_* calls: every one of them is a session call under UIS_RULE_STREAM_OTHER (a pending
// uis_min_turn table is a decode's, and is refused here as by every uis_stream_* call)
int begin_session_call(uis_handle* h, const char* who) { return begin_call(h, who, UIS_RULE_STREAM_OTHER); }

}  // namespace

// A value may differ from the slot's current one only while the slot's utterance has received nothing: the run of a
// live hypothesis saturates at the value it was formed under.  All or nothing.  A session call between launches: the
// resident launch of a UIS_FLAG_PERSISTENT session leaves, and the next push's launch is given the new pointer.
UIS_EXPORT int32_t uis_session_min_turn(uis_handle* h, const int32_t* min_turn) {
  if (int rc = begin_session_call(h, "uis_session_min_turn")) return rc;
  if (!session_of(h, min_turn != nullptr, "null handle/min_turn")) return UIS_ERR_INVALID_ARG;
  uis_handle::Stream& ss = h->stream_state;
  bool any = false, changed = false;
  for (int u = 0; u < ss.U; ++u) {
    if (min_turn[u] < 0 || min_turn[u] > UIS_MIN_TURN_MAX)
      return fail(UIS_ERR_INVALID_ARG, "a minimum turn length must be in [0, 32767] (0 and 1: no rule)");
    if (min_turn[u] != ss.min_turn[u] && ss.committed[u] + ss.have[u] != 0)
      return fail(UIS_ERR_INVALID_ARG, "utterance " + std::to_string(u) + " has already received or been primed with " +
                                           std::to_string((long long)(ss.committed[u] + ss.have[u])) +
                                           " frames: its slot's minimum turn length changes only before the first frame "
                                           "(after uis_stream_begin or uis_stream_restart); nothing was changed");
    any = any || min_turn[u] >= 2;
    changed = changed || min_turn[u] != ss.min_turn[u];
  }
  if (!changed) return UIS_OK;
  if (int rc = session_enter(h, nullptr)) return rc;  // (the resident launch leaves: the table is written between launches)
  const std::vector<int32_t> next(min_turn, min_turn + ss.U);
  HIPCHK(hipMemcpyAsync(ss.d_min_turn, next.data(), (size_t)ss.U * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  ss.min_turn = next;
  ss.st.min_turn = any ? ss.d_min_turn : nullptr;
  return UIS_OK;
}

UIS_EXPORT int32_t uis_session_get_min_turn(uis_handle* h, int32_t* out) {
  if (int rc = begin_session_call(h, "uis_session_get_min_turn")) return rc;
  if (!session_of(h, out != nullptr, "null handle/out")) return UIS_ERR_INVALID_ARG;
  const uis_handle::Stream& ss = h->stream_state;
  for (int u = 0; u < ss.U; ++u) out[u] = ss.min_turn[u];
  return UIS_OK;
}

namespace {

#define UIS_TURNS_THREADS 64

// The turn the best hypothesis is in, one thread per utterance (two loads and two stores each: a workgroup per
// utterance, as k_stream_bindings has for its 128 output words, would idle 63 lanes of 64), between launches: out[u] = {the label of rank 0's
// last-label word -- a cluster index as uis_stream_labels numbers them now --, its run}.  The run is 0 where the slot
// has no rule (such a word carries none); {-1, 0} for an utterance without a live hypothesis (an emptied beam, the
// overflow word set) and for one that has received nothing.  A window that a commit emptied keeps its one hypothesis.
__global__ __launch_bounds__(UIS_TURNS_THREADS) void k_session_turns(DecodeState st, int32_t* __restrict__ out) {
  const int u = blockIdx.x * UIS_TURNS_THREADS + threadIdx.x;
  if (u >= st.U) return;
  const auto [N, T, par, nb, live, e, bp] = beam_view(st, u, EMPTY_WINDOW_KEEPS_BEAM);
  int label = -1, run = 0;
  if (live > 0) {
    const int w = st.beam_last[e];   // rank 0
    const int K = st.beam_K[e];
    if (w >= 0 && last_label(w) >= 0 && last_label(w) < K) {
      label = last_label(w);
      run = utt_min_turn(st, u) >= 2 ? last_run(w) : 0;
    }
  }
  out[2 * (size_t)u] = label;
  out[2 * (size_t)u + 1] = run;
}

}  // namespace

// May the speaker change at the next frame: see include/uisrnn_hip.h.  The scaffold's order; nothing of the session changes.
UIS_EXPORT int32_t uis_session_turns(uis_handle* h, int32_t* out) {
  if (int rc = begin_session_call(h, "uis_session_turns")) return rc;
  if (!session_of(h, out != nullptr, "null handle/out")) return UIS_ERR_INVALID_ARG;
  const int U = h->stream_state.U;
  return session_query(h, "uis_session_turns", "UIS_TURNS_TRACE", (size_t)U * 8, out, [&](const DecodeState& stv, int32_t* d_out) {
    hipLaunchKernelGGL(k_session_turns, dim3((U + UIS_TURNS_THREADS - 1) / UIS_TURNS_THREADS), dim3(UIS_TURNS_THREADS), 0, h->stream, stv, d_out);
  });
}

namespace {

#define UIS_PROFILES_THREADS 256

// The speakers of the best hypothesis, one workgroup per utterance, threads over (cluster,
// dimension), between launches.  Rank 0 of the final beam holds K clusters; cluster k -- the numbering uis_stream_labels
// uses right now -- lives in pool slot beam_slot[k]: n[u] = K, stats[u][k] = {pool_cnt of the slot, the count and the
// tag of the block-count word, 0}, mean[u][k] = the D real dimensions of the slot's pool_mean row.  Rows k >= K:
// {0, 0, -1, -1} and +0.0.  n[u] = -1 and every row absent for an utterance without a live hypothesis (an emptied beam,
// the overflow word set); 0 for one that has received nothing.  A window that a commit emptied keeps its one hypothesis.
__global__ __launch_bounds__(UIS_PROFILES_THREADS) void k_session_profiles(DevModel m, DecodeState st, int width, int32_t* __restrict__ n_out,
                                                                           int4* __restrict__ stats, float* __restrict__ mean) {
  const int u = blockIdx.x, tid = threadIdx.x;
  if (u >= st.U) return;
  const auto [N, T, par, nb, live, e, bp] = beam_view(st, u, EMPTY_WINDOW_KEEPS_BEAM);
  int K = -1;
  if (live > 0) {
    K = st.beam_K[e];   // rank 0
    const int cap = st.Kmax < width ? st.Kmax : width;
    K = K < 0 ? 0 : (K > cap ? cap : K);
  }
  if (tid == 0) n_out[u] = K;
  const int32_t* slot = st.beam_slot + e * st.Kmax;
  const int32_t* blk = st.beam_blk + e * st.Kmax;
  for (int k = tid; k < width; k += UIS_PROFILES_THREADS) {
    int4 v = make_int4(0, 0, -1, -1);
    if (k < K) {
      const int sl = slot[k], w = blk[k];
      v = make_int4(sl >= 0 && sl < st.S ? st.pool_cnt[(size_t)u * st.S + sl] : 0, blk_count(w), blk_tag(w), 0);
    }
    stats[(size_t)u * width + k] = v;
  }
  const int total = width * m.D;
  for (int idx = tid; idx < total; idx += UIS_PROFILES_THREADS) {
    const int k = idx / m.D, d = idx - k * m.D;
    float v = 0.0f;
    if (k < K) {
      const int sl = slot[k];
      if (sl >= 0 && sl < st.S) v = st.pool_mean[((size_t)u * st.S + sl) * m.Dp + d];
    }
    mean[(size_t)u * total + idx] = v;
  }
}

}  // namespace

// Who the best hypothesis' speakers are right now: see include/uisrnn_hip.h.  The scaffold's order; nothing of the
// session changes.  One output block {n [U], stats [U][width][4], mean [U][width][D]}, split on the host.
UIS_EXPORT int32_t uis_session_profiles(uis_handle* h, int32_t width, int32_t* n_clusters_out, int32_t* stats_out, float* mean_out) {
  if (int rc = begin_session_call(h, "uis_session_profiles")) return rc;
  if (!session_of(h, n_clusters_out && stats_out && mean_out, "null handle/n_clusters_out/stats_out/mean_out")) return UIS_ERR_INVALID_ARG;
  const uis_handle::Stream& ss = h->stream_state;
  const int U = ss.U, D = h->m.D;
  if (width < ss.Kmax)
    return fail(UIS_ERR_INVALID_ARG, "width must be at least the session's max_clusters (" + std::to_string(ss.Kmax) + "), not " +
                                         std::to_string(width));
  if ((int64_t)U * width * (D + 4) > 0x1fffffffLL) return fail(UIS_ERR_UNSUPPORTED, "the profiles of one call exceed 2 GB: a smaller width");
  const size_t rows = (size_t)U * width;
  const size_t o_stats = ((size_t)U * 4 + 15) & ~(size_t)15, o_mean = o_stats + rows * 16, bytes = o_mean + rows * D * 4;
  std::vector<char> block(bytes);
  const DevModel m = h->m;
  int rc = session_query(h, "uis_session_profiles", "UIS_PROFILES_TRACE", bytes, block.data(), [&](const DecodeState& stv, int32_t* d_out) {
    char* base = reinterpret_cast<char*>(d_out);
    hipLaunchKernelGGL(k_session_profiles, dim3(U), dim3(UIS_PROFILES_THREADS), 0, h->stream, m, stv, (int)width, d_out,
                       reinterpret_cast<int4*>(base + o_stats), reinterpret_cast<float*>(base + o_mean));
  });
  if (rc) return rc;
  memcpy(n_clusters_out, block.data(), (size_t)U * 4);
  memcpy(stats_out, block.data() + o_stats, rows * 16);
  memcpy(mean_out, block.data() + o_mean, rows * D * 4);
  return UIS_OK;
}
