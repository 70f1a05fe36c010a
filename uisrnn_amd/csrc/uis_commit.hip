// uis_commit.hip -- uis_stream_commit: hand out the labels of a session that are final, drop their back-pointers and
// give the room back to the session, so that a stream of any length is decoded in a window of max_frames frames.
//
// Between two pushes a session is its tables (uis_prime.hip's header comment names them and who reads them again).
// Of these only bp -- one [B] row of records per frame, label | parent << 16 -- grows with the stream; the slot
// pool, pool_cnt, the beam tables and their block counts are sums over everything the utterance ever received and
// do not know where the window starts.  So a commit is three small steps, between launches, no decode kernel:
//   the readout   k_nbest as uis_stream_nbest(1) launches it: rank 0's labels of the window and the STABLE PREFIX,
//                 the leading frames on which all live hypotheses share one ancestor (those labels are final)
//   the prune     k_commit_prune: with a decision horizon, cut = max(stable, have - horizon) and every live
//                 hypothesis whose ancestor at step cut - 1 is not rank 0's leaves the beam; the survivors move up
//                 to ranks 0 .. n' - 1 in order -- their scalars, their slot / block lists and their record of the
//                 last step (the one table indexed by the CURRENT ranks).  Nothing else refers to a rank: free
//                 slots are found from the live beam at every step, and 1 <= beam_n < B is how every session starts.
//                 After it all survivors share one ancestor at step cut - 1: cut is the new stable prefix
//   the move      k_commit_move: c = cut & ~1 rows leave the front of the utterance's records, rows [c, have) go to
//                 [0, have - c), utt_step -= c.  c is even, so the live beam tables keep the parity of utt_step.
// An utterance that has nothing in its window, whose beam is empty or which is flagged in the overflow word
// commits 0 and is not touched.
//
// The prior tables logblk / logden are indexed by block counts and their sum, which go on growing with the stream:
// before anything is launched the call makes sure they reach (frames ever received) + max_frames + 2 entries and
// uploads longer ones (at least twice the length, upload_log_tables' arithmetic: the common prefix keeps its bits)
// where they do not; the session is pointed at them after the synchronisation and the old ones are freed then.
//
// The order is the scaffold's (uis_stream.hip); this call's own: the longer prior tables are allocated before any
// scratch (an allocation that fails leaves the session as it was) and swapped in after the synchronisation.
//
// #included by uis_decoder.hip after uis_stream.hip (the scaffold) and uis_nbest.hip (k_nbest).

namespace {

struct CommitArgs {
  const int32_t* horizon;    // [U] or null: no decision horizon
  const long long* stable;   // [U] k_nbest's stable prefix
  int32_t* cut_even;         // [U] out: frames committed (c)
  int32_t* dropped;          // [U] out: hypotheses pruned
};

// One workgroup per utterance.  st.avail = the window's frame counts (the host's `have`).
__global__ __launch_bounds__(UIS_COMMIT_THREADS) void k_commit_prune(DecodeState st, CommitArgs a) {
  __shared__ int s_anc[256];   // rank r's ancestor at step cut - 1
  __shared__ int s_src[256];   // the survivor that becomes rank j
  __shared__ int s_n;
  const int u = blockIdx.x, tid = threadIdx.x;
  if (u >= st.U) return;
  const int B = st.B, Kmax = st.Kmax;
  const auto [N, T, par, nb, live, e, bp] = beam_view(st, u);
  if (live == 0) {                            // nothing received, an emptied beam, the cluster cap: left alone
    if (tid == 0) { a.cut_even[u] = 0; a.dropped[u] = 0; }
    return;
  }
  long stab = (long)a.stable[u];
  stab = stab < 0 ? 0 : (stab > N ? N : stab);
  long cut = stab;
  const int hz = a.horizon ? a.horizon[u] : -1;
  if (hz >= 0 && N - (long)hz > cut) cut = N - (long)hz;
  if (tid == 0) a.cut_even[u] = (int32_t)(cut & ~1L);
  if (cut <= stab) {                          // no prune: every live hypothesis already shares the ancestor
    if (tid == 0) a.dropped[u] = 0;
    return;
  }
  // ---- every live rank's ancestor at step cut - 1: its chain through steps N - 1 .. cut
  if (tid < live) {
    int r = tid;
    for (long s = N - 1; s >= cut; --s) r = rec_parent(bp[(size_t)s * B + r], B);  // (stale words are never reached from a live rank)
    s_anc[tid] = r;
  }
  __syncthreads();
  const bool keep = tid < live && s_anc[tid] == s_anc[0];
  int dest = 0;
  if (tid < live)
    for (int r = 0; r < tid; ++r) dest += s_anc[r] == s_anc[0] ? 1 : 0;
  if (keep) s_src[dest] = tid;
  if (tid == live - 1) s_n = dest + (keep ? 1 : 0);
  // ---- the scalars and the last step's record: read everything, barrier, write (destination ranks overlap sources)
  int32_t vK = 0, vlast = 0, vsum = 0;
  float vscore = 0.0f;
  uint32_t vbp = 0;
  if (keep) {
    vK = st.beam_K[e + tid]; vlast = st.beam_last[e + tid]; vsum = st.beam_sum[e + tid]; vscore = st.beam_score[e + tid];
    vbp = bp[(size_t)(N - 1) * B + tid];
  }
  loads_before_stores();
  if (keep) {
    st.beam_K[e + dest] = vK; st.beam_last[e + dest] = vlast; st.beam_sum[e + dest] = vsum; st.beam_score[e + dest] = vscore;
    bp[(size_t)(N - 1) * B + dest] = vbp;
  }
  // ---- the slot / block lists, rank by rank upwards.  Survivor j comes from rank src(j) >= j and src is increasing,
  // so row j is written after every read of it (by src(j') = j only for j' <= j) and entry k of every row is handled
  // by the same thread, in program order: no barrier is needed between the rows.
  const int n2 = s_n;
  for (int j = 0; j < n2; ++j) {
    const int src = s_src[j];
    if (src == j) continue;
    for (int k = tid; k < Kmax; k += UIS_COMMIT_THREADS) {
      st.beam_slot[(e + j) * Kmax + k] = st.beam_slot[(e + src) * Kmax + k];
      st.beam_blk[(e + j) * Kmax + k] = st.beam_blk[(e + src) * Kmax + k];
    }
  }
  if (tid == 0) {
    st.beam_n[(size_t)par * st.U + u] = n2;
    a.dropped[u] = live - n2;
  }
}

// One workgroup per utterance: rows [c, N) of its records move to [0, N - c), then utt_step -= c.  Source and
// destination overlap whenever N - c > c: move_words_down (uis_beam_view.h).
__global__ __launch_bounds__(UIS_COMMIT_THREADS) void k_commit_move(DecodeState st, const int32_t* __restrict__ cut_even) {
  const int u = blockIdx.x;
  if (u >= st.U) return;
  const int c = cut_even[u];
  if (c <= 0) return;
  const long N = (long)st.avail[u];
  uint32_t* dst = st.bp + (size_t)st.tau * st.off[u] * st.B;
  move_words_down(dst, dst + (size_t)c * st.B, (N - c) * (long)st.B);
  if (threadIdx.x == 0) st.utt_step[u] -= c;
}

}  // namespace

UIS_EXPORT int32_t uis_stream_commit(uis_handle* h, const int32_t* horizon, int32_t* labels_out, int64_t capacity,
                                     int32_t* counts_out, int32_t* dropped_out) {
  if (int rc = begin_call(h, "uis_stream_commit", UIS_RULE_STREAM_OTHER)) return rc;
  if (!session_of(h, counts_out != nullptr, "null handle/counts_out")) return UIS_ERR_INVALID_ARG;
  uis_handle::Stream& ss = h->stream_state;
  const int U = ss.U, B = ss.B;
  CallTimer timer{h};
  // ---- the checks
  const std::vector<int64_t> off = window_offsets(ss);
  int64_t most = 0;  // frames any utterance can have received once its window is full again
  for (int u = 0; u < U; ++u) most = std::max<int64_t>(most, ss.committed[u] + ss.have[u]);
  const int64_t F = off[U];
  if (capacity < F)
    return fail(UIS_ERR_INVALID_ARG, "labels_out: " + std::to_string((long long)F) + " int32 slots needed (the frames in the window)");
  if (F > 0 && !labels_out) return fail(UIS_ERR_INVALID_ARG, "labels_out is null");
  if (F == 0) {
    std::fill(counts_out, counts_out + U, 0);
    if (dropped_out) std::fill(dropped_out, dropped_out + U, 0);
    return UIS_OK;
  }
  int rc;
  DecodeState stc;
  if ((rc = session_enter(h, &stc))) return rc;
  hipStream_t st = h->stream;
  // ---- the prior tables: long enough for whatever the window can hold after this call
  PriorTableGrowth prior;
  if ((rc = prior.reserve(h, most + ss.cap + 2))) return rc;
  // ---- scratch: [horizon U], then [committed U][dropped U][rank 0's score U] as one stretch (they come back in one copy)
  ScratchPlan plan;
  const size_t o_hz = plan.take((size_t)U * 4), o_cut = plan.take((size_t)U * 4), o_drop = plan.take((size_t)U * 4, 4),
               o_score = plan.take((size_t)U * 4, 4);
  if ((rc = h->nb_labels.ensure((size_t)F * 4))) return rc;
  if ((rc = h->nb_stable.ensure((size_t)U * 8))) return rc;
  if ((rc = h->nb_off.ensure((size_t)U * 8))) return rc;
  char* base;  // (the pinned landing block: labels, then the three words per utterance)
  if ((rc = session_buffers(h, plan, ((size_t)F + 3 * (size_t)U) * 4, &base, {&h->nb_labels, &h->nb_stable, &h->nb_off, &prior.blk, &prior.den})))
    return rc;
  if ((rc = prior.upload(h))) return rc;
  if (horizon) HIPCHK(hipMemcpyAsync(base + o_hz, horizon, (size_t)U * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(h->nb_off.p, off.data(), (size_t)U * 8, hipMemcpyHostToDevice, st));
  CommitArgs a{};
  a.horizon = horizon ? reinterpret_cast<const int32_t*>(base + o_hz) : nullptr;
  a.stable = h->nb_stable.as<long long>();
  a.cut_even = reinterpret_cast<int32_t*>(base + o_cut);
  a.dropped = reinterpret_cast<int32_t*>(base + o_drop);
  // ---- readout, prune, move
  HIPCHK(timer.begin());
  hipLaunchKernelGGL(k_nbest, dim3(U), dim3(UIS_NBEST_THREADS), nbest_lds_bytes(B), st, stc, 1, h->nb_off.as<int64_t>(),
                     h->nb_labels.as<int32_t>(), reinterpret_cast<float*>(base + o_score), (int32_t*)nullptr,
                     h->nb_stable.as<long long>());
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_commit_prune, dim3(U), dim3(UIS_COMMIT_THREADS), 0, st, stc, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_commit_move, dim3(U), dim3(UIS_COMMIT_THREADS), 0, st, stc, (const int32_t*)a.cut_even);
  HIPCHK(hipGetLastError());
  HIPCHK(timer.end());
  int32_t* h_lab = ss.h_land.as<int32_t>();
  int32_t* h_cut = h_lab + F;
  int32_t* h_drop = h_cut + U;
  const float* h_score = reinterpret_cast<const float*>(h_drop + U);  // rank 0's score: it survives every prune
  HIPCHK(hipMemcpyAsync(h_lab, h->nb_labels.p, (size_t)F * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(h_cut, a.cut_even, (size_t)3 * U * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  // ---- the host's side of the move
  int64_t out = 0;
  for (int u = 0; u < U; ++u) {
    const int32_t c = h_cut[u];
    std::copy(h_lab + off[u], h_lab + off[u] + c, labels_out + out);
    out += c;
    counts_out[u] = c;
    if (dropped_out) dropped_out[u] = h_drop[u];
    ss.have[u] -= c;
    ss.committed[u] += c;
    if (c > 0) ss.win_score[u] = h_score[u];
  }
  prior.swap(h);
  h->nb_valid = false;
  if (CallTimer::env("UIS_COMMIT_TRACE"))
    fprintf(stderr, "uis_stream_commit: utterances %d window_frames %lld committed %lld prior_table_entries %lld device_ms %.3f call_ms %.3f\n",
            U, (long long)F, (long long)out, (long long)ss.log_len, timer.device_ms(), timer.call_ms());
  return UIS_OK;
}

UIS_EXPORT int32_t uis_stream_committed(uis_handle* h, int64_t* committed_out) {
  if (int rc = begin_call(h, "uis_stream_committed", UIS_RULE_STREAM_OTHER)) return rc;
  if (!session_of(h, committed_out != nullptr, "null handle/committed_out")) return UIS_ERR_INVALID_ARG;
  uis_handle::Stream& ss = h->stream_state;
  std::copy(ss.committed.begin(), ss.committed.end(), committed_out);
  return UIS_OK;
}
