// uis_restart.hip -- uis_stream_restart: end some utterances of a live session, hand out their final window labels
// and leave their slots as uis_stream_begin leaves an utterance, without touching the neighbours.
//
// Between two pushes an utterance is its tables (uis_prime.hip's header comment names them and who reads them again):
// utt_step, overflow, beam_n of both parities, the beam tables, its S pool slots and its bp rows.  No free list
// persists and every push rebuilds nrows / rows / gi_up / a1 / the control words, so "fresh" is what k_init_state
// writes for an utterance and nothing more: utt_step = 0, overflow = 0, beam_n = {1, 0}, rank 0 of the parity-0 beam
// scalars = the empty hypothesis of score 0.  Everything else of the slot is dead memory that the next stream
// defines before it reads it, exactly as in a session that has just been opened.  So a restart is two small steps,
// between launches, no decode kernel:
//   the readout   k_backtrace as uis_stream_labels launches it, with avail = the window's frame count for the
//                 utterances that end and 0 for the others (which then cost nothing and download nothing)
//   the reset     k_stream_restart: the selected utterances' overflow words are saved, then the words above are
//                 written.  nrows / counters belong to the session and are not touched
// UIS_POISON_WORKSPACE: k_stream_restart_fill runs between the two and fills everything the ended stream leaves
// behind in the slot -- its bp rows, its pool slots (mean, hidden states, frame counts) and its rows of the beam
// tables of both parities -- so that a recycled slot provably depends on nothing of its previous tenant.
//
// The order is the scaffold's (uis_stream.hip); this call's own: the readout's avail is its own table in the scratch
// (not the session's d_have), and a call that selects nothing still prints its trace line.
//
// #included by uis_decoder.hip after uis_commit.hip.

namespace {

#define UIS_RESTART_THREADS 256

// One thread per utterance.  overflow_out: the word before the reset (0 for an utterance not selected).
__global__ __launch_bounds__(UIS_RESTART_THREADS) void k_stream_restart(DecodeState st, const int32_t* __restrict__ which,
                                                                        int32_t* __restrict__ overflow_out) {
  const int u = blockIdx.x * UIS_RESTART_THREADS + threadIdx.x;
  if (u >= st.U) return;
  if (!which[u]) { overflow_out[u] = 0; return; }
  overflow_out[u] = st.overflow[u];
  st.utt_step[u] = 0;
  st.overflow[u] = 0;
  st.beam_n[u] = 1;            // parity 0
  st.beam_n[st.U + u] = 0;
  const size_t e = (size_t)u * st.B;
  st.beam_K[e] = 0; st.beam_last[e] = -1; st.beam_sum[e] = 0; st.beam_score[e] = 0.0f;
}

__device__ __forceinline__ void restart_fill(void* p, size_t first, size_t count, uint32_t word) {
  uint32_t* w = static_cast<uint32_t*>(p) + first;
  for (size_t i = threadIdx.x; i < count; i += UIS_RESTART_THREADS) w[i] = word;
}

// One workgroup per utterance: what the ended stream leaves behind in a selected slot, filled with `word`.
// Dp / Hp / depth: the pool's row layout (DevModel's).
__global__ __launch_bounds__(UIS_RESTART_THREADS) void k_stream_restart_fill(DecodeState st, const int32_t* __restrict__ which,
                                                                             int Dp, int Hp, int depth, uint32_t word) {
  const int u = blockIdx.x;
  if (u >= st.U || !which[u]) return;
  const size_t B = (size_t)st.B, S = (size_t)st.S, Kmax = (size_t)st.Kmax;
  restart_fill(st.bp, (size_t)st.tau * st.off[u] * B, (size_t)st.tau * (size_t)(st.off[u + 1] - st.off[u]) * B, word);
  restart_fill(st.pool_mean, (size_t)u * S * Dp, S * Dp, word);
  restart_fill(st.pool_hid, (size_t)u * S * depth * Hp, S * depth * Hp, word);
  restart_fill(st.pool_cnt, (size_t)u * S, S, word);
  for (int par = 0; par < 2; ++par) {
    const size_t e = ((size_t)par * st.U + u) * B;
    restart_fill(st.beam_K, e, B, word);
    restart_fill(st.beam_last, e, B, word);
    restart_fill(st.beam_sum, e, B, word);
    restart_fill(st.beam_score, e, B, word);
    restart_fill(st.beam_slot, e * Kmax, B * Kmax, word);
    restart_fill(st.beam_blk, e * Kmax, B * Kmax, word);
    restart_fill(st.beam_n, (size_t)par * st.U + u, 1, word);
  }
  restart_fill(st.utt_step, (size_t)u, 1, word);
}

}  // namespace

UIS_EXPORT int32_t uis_stream_restart(uis_handle* h, const int32_t* which, int32_t* labels_out, int64_t capacity,
                                      int32_t* counts_out, float* scores_out, int32_t* overflow_out) {
  if (int rc = begin_call(h, "uis_stream_restart", UIS_RULE_STREAM_OTHER)) return rc;
  if (!session_of(h, which && counts_out, "null handle/which/counts_out")) return UIS_ERR_INVALID_ARG;
  uis_handle::Stream& ss = h->stream_state;
  const int U = ss.U;
  CallTimer timer{h};
  // ---- the checks
  int n_sel = 0;
  int64_t F = 0;
  for (int u = 0; u < U; ++u)
    if (which[u]) { ++n_sel; F += ss.have[u]; }
  if (capacity < F)
    return fail(UIS_ERR_INVALID_ARG, "labels_out: " + std::to_string((long long)F) + " int32 slots needed (the window frames of the utterances that end)");
  if (F > 0 && !labels_out) return fail(UIS_ERR_INVALID_ARG, "labels_out is null");
  // UIS_RESTART_TRACE: one line per call on stderr (read per call: a test turns it on)
  auto trace = [&] {  // (also for a call that selects nothing)
    if (CallTimer::env("UIS_RESTART_TRACE"))
      fprintf(stderr, "uis_stream_restart: utterances %d selected %d labels %lld device_ms %.3f call_ms %.3f persistent %d resident_launches %lld\n",
              U, n_sel, (long long)F, timer.device_ms(), timer.call_ms(), ss.persist ? 1 : 0, (long long)ss.pm_launches);
  };
  if (n_sel == 0) {
    std::fill(counts_out, counts_out + U, 0);
    trace();
    return UIS_OK;
  }
  int rc;
  if ((rc = session_enter(h, nullptr))) return rc;  // (the readout's avail is this call's own table: the utterances that end)
  hipStream_t st = h->stream;
  // ---- scratch: [which U][avail U][label offsets U] go up in one copy, [scores U][overflow U][labels F] come back in one
  ScratchPlan plan;
  const size_t o_which = plan.take((size_t)U * 4), o_avail = plan.take((size_t)U * 4, 4), o_laboff = plan.take((size_t)U * 8),
               o_score = plan.take((size_t)U * 4, 4), o_over = plan.take((size_t)U * 4, 4), o_lab = plan.take((size_t)F * 4, 4),
               land = plan.total - o_score;
  char* base;
  UisPoison poison;
  if ((rc = session_buffers(h, plan, land, &base, {}, &poison))) return rc;
  std::vector<char> up(o_score, 0);
  {
    int32_t* w = reinterpret_cast<int32_t*>(up.data() + o_which);
    int32_t* a = reinterpret_cast<int32_t*>(up.data() + o_avail);
    int64_t* lo = reinterpret_cast<int64_t*>(up.data() + o_laboff);
    int64_t pos = 0;
    for (int u = 0; u < U; ++u) {
      w[u] = which[u] ? 1 : 0;
      a[u] = which[u] ? ss.have[u] : 0;  // frames in the window = steps run since the last commit, from the host's own count
      lo[u] = pos;
      pos += a[u];
    }
  }
  HIPCHK(hipMemcpyAsync(base, up.data(), o_score, hipMemcpyHostToDevice, st));
  const int32_t* d_which = reinterpret_cast<const int32_t*>(base + o_which);
  DecodeState stl = ss.st;
  stl.avail = reinterpret_cast<const int32_t*>(base + o_avail);
  stl.lab_off = reinterpret_cast<const int64_t*>(base + o_laboff);
  // ---- readout, reset
  HIPCHK(timer.begin());
  hipLaunchKernelGGL(k_backtrace, dim3(U), dim3(64), (size_t)64 * ss.B, st, stl, reinterpret_cast<int32_t*>(base + o_lab),
                     reinterpret_cast<float*>(base + o_score), (float*)nullptr);
  HIPCHK(hipGetLastError());
  if (poison.on) {
    hipLaunchKernelGGL(k_stream_restart_fill, dim3(U), dim3(UIS_RESTART_THREADS), 0, st, ss.st, d_which, h->m.Dp, h->m.Hp,
                       h->m.depth, poison.word);
    HIPCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_stream_restart, dim3((U + UIS_RESTART_THREADS - 1) / UIS_RESTART_THREADS), dim3(UIS_RESTART_THREADS), 0, st,
                     ss.st, d_which, reinterpret_cast<int32_t*>(base + o_over));
  HIPCHK(hipGetLastError());
  HIPCHK(timer.end());
  HIPCHK(hipMemcpyAsync(ss.h_land.p, base + o_score, land, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  // ---- the host's side
  const float* h_score = ss.h_land.as<float>();
  const int32_t* h_over = reinterpret_cast<const int32_t*>(h_score + U);
  const int32_t* h_lab = h_over + U;
  if (F > 0) std::copy(h_lab, h_lab + F, labels_out);
  int n_over = 0;
  for (int u = 0; u < U; ++u) {
    if (!which[u]) { counts_out[u] = 0; continue; }
    counts_out[u] = ss.have[u];
    // (a window that a commit emptied still has its one hypothesis and its score: uis_stream_labels' rule)
    if (scores_out) scores_out[u] = ss.window_emptied(u) ? ss.win_score[u] : h_score[u];
    if (overflow_out) overflow_out[u] = h_over[u];
    n_over += h_over[u] != 0;
    ss.have[u] = 0;
    ss.committed[u] = 0;
    ss.win_score[u] = 0.0f;
  }
  h->nb_valid = false;
  trace();
  return cluster_cap_status(n_over, ss.Kmax);
}
