// uis_workspace.hip -- the decode state's memory, described once (included by uis_decoder.hip).
//
//   state_counts()      element counts of the tables a DecodeState needs whoever allocates them: the offline decode
//                       (workspace_list, views into the arena) and a session (uis_stream_begin, its own allocations)
//   wire_cluster_ctl()  a DecodeState's control pointers from a control-word block and a ClusterGeometry
//   upload_log_tables() logblk / logden
//   workspace_list()    the ordered (buffer, bytes) list of one offline decode
//   place_workspace()   that list into the arena, or into allocations of their own with k_decode_rs's one stretch
//
// A kernel that needs one more table or word: a line in state_counts (if sessions need it too) and a line in
// workspace_list, in the place the layout wants it.

namespace {

// control words: [0, 16) XCC id per cluster, [16] abort, [32, 32 + 32 ncl) row counters,
// then 32 ncl barrier counters, then 32 ncl phase words (one 128-byte line per cluster each)
constexpr size_t kCtlWords = (size_t)32 + 3 * UIS_MAX_CLUSTERS * 32;

struct StateCounts {
  size_t pool_mean, pool_hid, pool_cnt;  // float, float, int32
  size_t beam_n;                         // int32
  size_t beam;                           // each of beam_K, beam_last, beam_sum (int32) and beam_score (float)
  size_t beam_lists;                     // each of beam_slot, beam_blk (int32)
  size_t rows, nrows;                    // RnnRow, int32
  size_t gi_up, a1;                      // float
  size_t ctl_words;                      // uint32
};

// `groups`: utterance groups the state is shared by (two row counters each).
StateCounts state_counts(const DevModel& m, int U, int B, int Kmax, int S, long rows_cap, int groups) {
  StateCounts n;
  n.pool_mean = (size_t)U * S * m.Dp;
  n.pool_hid = ((size_t)U * S + 1) * m.depth * m.Hp;  // + the slot k_decode_resident keeps h1 in
  n.pool_cnt = (size_t)U * S;
  n.beam_n = (size_t)2 * U;
  n.beam = (size_t)2 * U * B;
  n.beam_lists = (size_t)2 * U * B * Kmax;
  n.rows = (size_t)rows_cap;
  n.nrows = (size_t)groups * 2;
  n.gi_up = m.depth > 1 ? (size_t)rows_cap * m.G : (size_t)rows_cap * m.Hp;  // depth 1: k_decode_resident's h' staging buffer
  n.a1 = (size_t)rows_cap * m.Hp;
  n.ctl_words = kCtlWords;
  return n;
}

// `geo` null: no cluster kernel runs on this state (the abort word is read back all the same).
void wire_cluster_ctl(DecodeState& st, uint32_t* ctl, const ClusterGeometry* geo) {
  st.cl_abort = ctl + 16;
  if (!geo) return;
  st.ncl = geo->ncl;
  st.cl_xcc = ctl;
  st.rx_stride = geo->rx_stride;
  st.rx_nrows = reinterpret_cast<int32_t*>(ctl) + 32;
  st.rx_bar = ctl + 32 + UIS_MAX_CLUSTERS * 32;
  st.rx_flags = ctl + 32 + 2 * UIS_MAX_CLUSTERS * 32;
}

// logblk[n] = log n and logden[n] = log(n + crp_alpha) for n < count, through `host` (which has to outlive the copies)
int upload_log_tables(double alpha, int64_t count, std::vector<double>& host, void* d_logblk, void* d_logden, hipStream_t stream) {
  host.resize((size_t)2 * count);
  for (int64_t n = 0; n < count; ++n) {
    host[n] = n > 0 ? std::log((double)n) : 0.0;       // np.log(block_counts[cluster]), uisrnn.py:418-419
    host[count + n] = std::log((double)n + alpha);     // np.log(sum(block_counts) + crp_alpha)
  }
  HIPCHK(hipMemcpyAsync(d_logblk, host.data(), (size_t)count * 8, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(d_logden, host.data() + count, (size_t)count * 8, hipMemcpyHostToDevice, stream));
  return UIS_OK;
}

struct WsItem { DevBuf* buf; size_t bytes; };
inline size_t ws_pad(size_t bytes) { return (bytes + 4095) & ~(size_t)4095; }  // every view starts on a 4 KB boundary
static const size_t kCtlPlace[4] = {0, 8192, (size_t)1 << 20, ((size_t)1 << 20) + 8192};  // uis_handle::CtlTune's candidates

// The workspace of one offline decode.  Every buffer is a 4 KB-aligned view into ONE allocation (h->arena), laid out in
// the order of this list -- which is part of the measured speed: keep the order and the sizes.
std::vector<WsItem> workspace_list(DecodeCall& c) {
  uis_handle* h = c.h;
  const DevModel& m = h->m;
  const DecodeShape& s = c.shape;
  const DecodePlan& plan = c.plan;
  const size_t U = (size_t)s.U, NC = (size_t)s.NC, frames = (size_t)std::max<int64_t>(s.F, 1);
  const int B = s.B, Kmax = s.Kmax, L = s.L;
  const StateCounts n = state_counts(m, s.U, B, Kmax, s.S, plan.rows_cap, UIS_MAX_GROUPS);
  std::vector<WsItem> want;
#define ENSURE(buf, bytes) want.push_back(WsItem{&h->buf, (size_t)(bytes)})
  ENSURE(off, (U + 1) * 8);  // (the utterances' frame offsets; a session's are capacity offsets)
  ENSURE(utt_step, U * 4);
  ENSURE(overflow, U * 4);
  if (m.D != m.Dp) ENSURE(xpad, frames * m.Dp * 4);
  ENSURE(gi0, frames * m.G * 4);
  ENSURE(mse0, frames * 4);
  // (k_decode_rs / k_decode_big<WS> copy the first UIS_RS_LOGTAB entries into LDS whatever the decode's length)
  c.n_log = std::max<int64_t>(s.maxT + 2, UIS_RS_LOGTAB);
  ENSURE(logblk, (size_t)c.n_log * 8);
  ENSURE(logden, (size_t)c.n_log * 8);
  ENSURE(pool_mean, n.pool_mean * 4);
  ENSURE(pool_hid, n.pool_hid * 4);
  ENSURE(pool_cnt, n.pool_cnt * 4);
  ENSURE(beam_n, n.beam_n * 4);
  ENSURE(beam_K, n.beam * 4);
  ENSURE(beam_last, n.beam * 4);
  ENSURE(beam_sum, n.beam * 4);
  ENSURE(beam_score, n.beam * 4);
  ENSURE(beam_slot, n.beam_lists * 4);
  ENSURE(beam_blk, n.beam_lists * 4);
  // (a record per decode step of the frames given; a session's: per frame of its capacity.  The window machinery
  // keeps its records in bp16)
  ENSURE(bp, !s.wnd ? (size_t)std::max<int64_t>(c.tau * s.F, 1) * B * 4 : 16);
  ENSURE(rows, n.rows * sizeof(RnnRow));
  ENSURE(nrows, n.nrows * 4);
  ENSURE(gi_up, n.gi_up * 4);
  ENSURE(a1, n.a1 * 4);
  // rnn_depth >= 2 in one launch (k_decode_deep): the two hand-off buffers a layer's h' goes through
  if (plan.hst) ENSURE(hst, (size_t)2 * plan.rows_cap * m.Hp * 4);
  // (four statistics words per group, then the diagnostic builds' clocks; a session has one group and no such build)
#if defined(UIS_RESIDENT_TIMING)
  ENSURE(counters, (size_t)UIS_MAX_GROUPS * 4 * 8 + (96 + 1024) * 8);
#else
  ENSURE(counters, (size_t)UIS_MAX_GROUPS * 4 * 8 + 96 * 8);
#endif
  ENSURE(beam_scores_out, U * B * 4);
  ENSURE(utt_nrows, U * 2 * 4);
  // (a decode in several launches: DecodeState::resume -- only lists given in host memory can split, and never through
  // the window machinery: wide beams, large caps and look-ahead decodes do not pay for it)
  ENSURE(resume, (c.h_frames && !s.wnd) ? U * (rs_lds_layout(B, Kmax, s.S).persist_stride + 4) + 16 : (size_t)16);
  ENSURE(split_tab, 8 * U * 2 * sizeof(long));     // (... of a ragged list: batch tables of up to 8 slices)
  ENSURE(scatter_tab, 64 * U * 3 * sizeof(long));  // (... and of its copy units: the scatter's tables)
  if (plan.stage) ENSURE(stage, (size_t)s.F * m.D * 4);  // (... the device's copy of the time-major staging block)
  ENSURE(cluster_ctl, kCtlPlace[3] + ws_pad(n.ctl_words * 4));
  c.mse_tab_bytes = ((size_t)2 * U * s.S * 4 + 255) & ~(size_t)255;
  c.mse_part_bytes = (size_t)plan.nclq * plan.rx_stride * rs_part_stride(m.Dp) * 4;
  if (c.rs) ENSURE(mse_tab, c.mse_tab_bytes + c.mse_part_bytes);
  if (c.dbg) ENSURE(dbg_scores, std::max<size_t>(c.dbg_floats, 1) * 4);
  if (s.wnd) {
    ENSURE(lv_n, 2 * U * 4);
    ENSURE(lv_K, 2 * U * NC * 4);
    ENSURE(lv_last, 2 * U * NC * 4);
    ENSURE(lv_sum, 2 * U * NC * 4);
    ENSURE(lv_score, 2 * U * NC * 4);
    ENSURE(lv_origin, 2 * U * NC * 4);
    ENSURE(lv_path, 2 * U * NC * L * 2);
    ENSURE(lv_slot, 2 * U * NC * Kmax * 4);
    ENSURE(lv_blk, 2 * U * NC * Kmax * 4);
    ENSURE(scratch, U * c.wsl.total);
    ENSURE(bp16, (size_t)std::max<int64_t>(c.bp_base[U], 1) * (L + 1) * 2);
    ENSURE(bp_base, (U + 1) * 8);
  }
  ENSURE(limit, U * 4);  // (last: every view above stays where it was measured)
  if (h->tables.limits.call_set) ENSURE(limit_in, U * 4);
  if (s.biased) ENSURE(bias3, frames * 24);  // (uis_frame_bias: {lp_stay, lp_sw, lp_new} per frame; behind everything, like the limits)
  if (s.hinted) ENSURE(hint, frames);  // (uis_frame_speakers: one tag per frame; behind everything above, so that none of it moves)
  if (s.turned) ENSURE(min_turn, U * 4);  // (uis_min_turn: one value per utterance; the very last view, likewise)
#undef ENSURE
  return want;
}

enum { WS_REPLAN = 1 };  // place_workspace: nothing placed, plan again without k_decode_rs

// Places the list: views into the arena (behind UIS_ARENA_SHIFT), or -- UIS_NO_ARENA -- an allocation per buffer with
// k_decode_rs's stretch still ONE, laid out as the arena would; then the poison fill.
// k_decode_rs names everything from pool_mean to the end of mse_tab by 32-bit offsets from pool_mean (RsArgs): that
// stretch of THIS list must stay below 4 GB -- it does unless the back-pointers of a very long list push it there,
// and then (WS_REPLAN) the planner's next kernel decodes.
int place_workspace(uis_handle* h, const DecodeKnobs& knobs, bool rs, const std::vector<WsItem>& want) {
  size_t rs_first = 1, rs_last = 0, rs_stretch = 0, total = 0;  // (an empty range without k_decode_rs)
  for (size_t i = 0; i < want.size(); ++i) {
    if (rs && want[i].buf == &h->pool_mean) rs_first = i;
    if (rs && want[i].buf == &h->mse_tab) rs_last = i;
    total += ws_pad(want[i].bytes);
  }
  for (size_t i = rs_first; i <= rs_last; ++i) rs_stretch += ws_pad(want[i].bytes);
  if (rs_stretch >= ((size_t)1 << 32)) return WS_REPLAN;
  // (UIS_ARENA_SHIFT, tools/experiments/bimodal.py: the one-launch decode runs in one of two modes
  // 4 % apart depending on where its buffers land)
  const bool arena = !knobs.no_arena;
  int rc;
  if ((rc = arena ? h->arena.ensure(total + knobs.arena_shift) : rs ? h->rs_block.ensure(rs_stretch) : UIS_OK)) return rc;
  size_t o = arena ? knobs.arena_shift : 0;
  for (size_t i = 0; i < want.size(); ++i) {
    if (arena || (i >= rs_first && i <= rs_last)) {
      want[i].buf->view(static_cast<char*>(arena ? h->arena.p : h->rs_block.p) + o, want[i].bytes);
      o += ws_pad(want[i].bytes);
    } else if ((rc = want[i].buf->ensure(want[i].bytes))) {
      return rc;
    }
  }
  // UIS_POISON_WORKSPACE: the whole placed arena (or every buffer of the list and k_decode_rs's stretch), on the
  // handle's stream ahead of ev_begin -- every other stream of this decode waits for that event (uis_poison.h)
  if (h->poison.on) {
    if (arena) HIPCHK(h->poison.device(h->arena.p, total + knobs.arena_shift, h->stream));
    else if (rs) HIPCHK(h->poison.device(h->rs_block.p, h->rs_block.cap, h->stream));
    for (const WsItem& w : want)
      if (!w.buf->borrowed) HIPCHK(h->poison.device(w.buf->p, w.buf->cap, h->stream));
  }
  return UIS_OK;
}

}  // namespace
