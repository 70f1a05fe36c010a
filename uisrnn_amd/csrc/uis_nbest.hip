// uis_nbest.hip -- n-best readout: trace[-N:] of EVERY hypothesis of the final beam, not only of rank 0.
//
// A decode leaves on the device the back-pointers of all beam_size ranks at every step and the final beam's
// scores; k_backtrace / k_backtrace_window (uis_kernels.hip) walk them from rank 0 only.  The kernels here walk
// from ranks 0 .. n-1 and nothing else: no decode kernel changes, the readout only reads what a decode left.
//
//   k_nbest         look_ahead 1 records (DecodeState::bp, label | parent << 16, [step][B], B <= 256), one
//                   workgroup per utterance:
//                     1. lane l of each wave owns segment l of the last N steps and follows every entry rank
//                        through it, 8 independent chains in flight (k_backtrace's phase 1; here the groups of 8
//                        ranks are dealt over the four waves) -> [64][B] byte map in LDS, exit rank by entry rank;
//                     2. thread k stitches hypothesis k: its entry rank at every segment -> [B][64] bytes in LDS;
//                     3. the (segment, hypothesis) pairs are dealt over all threads; each walks its segment once
//                        from its true entry rank and writes the labels.
//                   Sessions also get the STABLE PREFIX: the number of leading frames on which all live hypotheses
//                   have the same ancestor (every later beam descends from this one: those labels are final).
//                   From the stitched entries the latest segment boundary at which all live hypotheses enter by
//                   the same rank (a ballot over the lanes), then the segment above it with all live ranks in
//                   lock-step against rank 0's chain, down to the first step at which each has merged with it.
//   k_nbest_window  window records (DecodeState::bp16, {parent, c_1 .. c_L} per window and rank): one thread per
//                   (utterance, rank), the plain walk of k_backtrace_window.
// Both read the tables through uis_beam_view.h (k_backtrace's rules: avail for sessions and tau * N otherwise, the
// parity of T names the final beam, stale parent ranks are clamped to B - 1), take their output offsets from a table
// of the host's and fill the rows k >= count with -1; count = min(n, live hypotheses).
//
// Phases 1 and 2 of k_nbest are __device__ functions: k_posterior (uis_posterior.hip) starts from the same two.
//
// #included by uis_decoder.hip after uis_beam_view.h.

namespace {

#define UIS_NBEST_THREADS 256

// Phases 1 and 2 of k_nbest, shared with k_posterior (uis_posterior.hip); a workgroup of UIS_NBEST_THREADS threads,
// a __syncthreads() of the caller's after each.
// 1. lane l of each wave follows every entry rank through segment l (wave w: entry ranks 8 w .. 8 w + 7, then
//    + 32 ...) -> bt_map [64][B]
__device__ __forceinline__ void nbest_segment_maps(const uint32_t* __restrict__ bp, int B, const SegGeom& g, unsigned char* bt_map) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long hi = g.hi(lane), lo = g.lo(lane);
  if (lane < g.nseg) {
    unsigned char* mine = bt_map + (size_t)lane * B;
    for (int r0 = 8 * wave; r0 < B; r0 += 8 * (UIS_NBEST_THREADS / 64)) {
      int r[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) r[k] = r0 + k < B ? r0 + k : 0;
      for (long s2 = hi; s2 >= lo; --s2) {
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = rec_parent(bp[(size_t)s2 * B + r[k]], B);  // (stale entry ranks are never stitched in)
      }
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (r0 + k < B) mine[r0 + k] = (unsigned char)r[k];
    }
  }
}

// 2. stitch: hypothesis k's entry rank at every segment (B <= 256 = the workgroup's threads) -> ent [B][64]
__device__ __forceinline__ void nbest_stitch(int B, int live, int nseg, const unsigned char* bt_map, unsigned char* ent) {
  const int tid = threadIdx.x;
  if (tid < live) {
    int cur = tid;
    for (int l = 0; l < nseg; ++l) {
      ent[(size_t)tid * 64 + l] = (unsigned char)cur;
      cur = bt_map[(size_t)l * B + cur];
    }
  }
}

__global__ __launch_bounds__(UIS_NBEST_THREADS) void k_nbest(DecodeState st, int n, const int64_t* __restrict__ out_off,
                                                             int32_t* __restrict__ labels, float* __restrict__ scores,
                                                             int32_t* __restrict__ counts, long long* __restrict__ stable) {
  extern __shared__ __attribute__((aligned(16))) unsigned char nb_lds[];  // (NbestLds; its word: s_min)
  const int u = blockIdx.x;
  if (u >= st.U) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int B = st.B;
  const NbestLds lds = nbest_lds(nb_lds, B);
  int* s_min = lds.word;
  unsigned char *bt_map = lds.bt_map, *ent = lds.ent;
  const auto [N, T, par, nb, live, e, bp] = beam_view(st, u);
  const int cnt = live < n ? live : n;
  if (scores)
    for (int k = tid; k < n; k += UIS_NBEST_THREADS) scores[(size_t)u * n + k] = k < nb ? st.beam_score[e + k] : INFINITY;
  if (counts && tid == 0) counts[u] = cnt;
  if (tid == 0) *s_min = 0x7fffffff;
  int32_t* out = labels + out_off[u];
  for (long i = (long)cnt * N + tid; i < (long)n * N; i += UIS_NBEST_THREADS) out[i] = -1;
  const bool walk = N > 0 && live > 0;
  const SegGeom g = seg_geom(T, N);
  const int nseg = g.nseg;
  // ---- 1. the segment maps, 2. the stitch
  if (walk) nbest_segment_maps(bp, B, g, bt_map);
  __syncthreads();
  if (walk) nbest_stitch(B, live, nseg, bt_map, ent);
  __syncthreads();
  // ---- 3. the labels: pair p = (segment p / cnt, hypothesis p % cnt) -- neighbours read the same records' rows
  if (walk) {
    for (int p = tid; p < nseg * cnt; p += UIS_NBEST_THREADS) {
      const int l = p / cnt, k = p - l * cnt;
      int32_t* row = out + (long)k * N;
      walk_segment(bp, B, g, l, ent[(size_t)k * 64 + l], [row, f0 = T - N](long s2, uint32_t v) { row[s2 - f0] = (int32_t)rec_label(v); });
    }
  }
  // ---- the stable prefix (sessions)
  if (!stable) return;
  if (walk) {
    // the latest boundary all live hypotheses enter by the same rank (every wave finds it for itself)
    bool agree = lane < nseg;
    if (agree) {
      const int r0 = ent[lane];
      for (int k = 1; k < live; ++k) agree = agree && ent[(size_t)k * 64 + lane] == r0;
    }
    const unsigned long long mask = __ballot(agree);
    const int lstar = mask ? __ffsll((long long)mask) - 1 : nseg;
    if (lstar > 0 && tid < live) {
      // the segment above it: chain `tid` beside rank 0's chain, down to the step at which they have merged;
      // not inside the segment = at the boundary (one step below its lowest)
      const int sl = lstar - 1;
      const long h2 = g.hi(sl), l2 = g.lo(sl);
      int r = ent[(size_t)tid * 64 + sl], r0 = ent[sl];
      long merged = l2 - 1;
      for (long s2 = h2; s2 >= l2; --s2) {
        if (r == r0) { merged = s2; break; }
        r = rec_parent(bp[(size_t)s2 * B + r], B);
        r0 = rec_parent(bp[(size_t)s2 * B + r0], B);
      }
      atomicMin(s_min, (int)(merged + 1 - (T - N)));
    } else if (tid == 0) {
      atomicMin(s_min, (int)N);  // one live hypothesis: everything received is final
    }
  }
  __syncthreads();
  if (tid == 0) stable[u] = walk ? (long long)*s_min : 0ll;
}

// the window records: one thread per (utterance, rank)
__global__ __launch_bounds__(64) void k_nbest_window(DecodeState st, int n, const int64_t* __restrict__ out_off,
                                                     int32_t* __restrict__ labels, float* __restrict__ scores,
                                                     int32_t* __restrict__ counts) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)st.U * n) return;
  const int u = (int)(idx / n), k = (int)(idx - (long)u * n);
  const int L = st.L;
  const long N = (long)(st.off[u + 1] - st.off[u]);
  const long T = (long)st.tau * N;
  const long n_win = (T + L - 1) / L;
  const BeamView bv = beam_view_at(st, u, N, T, n_win, EMPTY_WINDOW_SHOWS_NOTHING);  // (the windows run name the parity)
  const int cnt = bv.live < n ? bv.live : n;
  if (scores) scores[(size_t)u * n + k] = k < bv.nb ? st.beam_score[bv.e + k] : INFINITY;
  if (counts && k == 0) counts[u] = cnt;
  if (N == 0) return;
  int32_t* out = labels + out_off[u] + (long)k * N;
  if (k >= cnt) { for (long i = 0; i < N; ++i) out[i] = -1; return; }
  int r = k;
  for (long w = n_win - 1; w >= 0; --w) {
    const long t0 = w * L;
    if (t0 + L <= T - N) break;
    const uint16_t* rec = st.bp16 + ((size_t)st.bp_base[u] + (size_t)w * st.B + r) * (L + 1);
    const int Lw = (int)((T - t0) < L ? (T - t0) : L);
    for (int j = 0; j < Lw; ++j) {
      const long tt = t0 + j;
      if (tt >= T - N) out[tt - (T - N)] = (int32_t)rec[1 + j];
    }
    r = (int)rec[0];
    if (r >= st.B) r = st.B - 1;  // records of windows that never ran (overflowed utterance) are stale
  }
}

// The readout of `groups` (each on its own DecodeState, utterances u0 ..) into the handle's nb_* buffers and on to
// the caller.  off: [U + 1] label offsets of the utterances; stable_out: sessions only.
int nbest_run(uis_handle* h, const std::vector<uis_handle::NbestGroup>& groups, bool wnd, int B, const std::vector<int64_t>& off,
              int32_t n_best, int32_t* labels_out, int64_t capacity, float* scores_out, int32_t* counts_out,
              int64_t* stable_out, std::vector<int32_t>* overflow) {
  const int U = (int)off.size() - 1;
  if (n_best < 1 || n_best > B)
    return fail(UIS_ERR_INVALID_ARG, "n_best must be in [1, beam_size = " + std::to_string(B) + "]");
  const int64_t F = U > 0 ? off[U] : 0;
  if (capacity < (int64_t)n_best * F)
    return fail(UIS_ERR_INVALID_ARG, "labels_out: " + std::to_string((long long)n_best * F) + " int32 slots needed");
  if (F > 0 && !labels_out) return fail(UIS_ERR_INVALID_ARG, "labels_out is null");
  if (U == 0) return UIS_OK;
  int rc;
  if ((rc = h->nb_labels.ensure((size_t)std::max<int64_t>(n_best * F, 1) * 4))) return rc;
  if ((rc = h->nb_scores.ensure((size_t)U * n_best * 4))) return rc;
  if ((rc = h->nb_counts.ensure((size_t)U * 4))) return rc;
  if ((rc = h->nb_stable.ensure((size_t)U * 8))) return rc;
  if ((rc = h->nb_off.ensure((size_t)U * 8))) return rc;
  {  // UIS_POISON_WORKSPACE: the readout's own buffers (what the decode or the session left behind is its input)
    const UisPoison poison = UisPoison::from_env();
    for (DevBuf* b : {&h->nb_labels, &h->nb_scores, &h->nb_counts, &h->nb_stable, &h->nb_off})
      HIPCHK(poison.device(b->p, b->cap, h->stream));
  }
  std::vector<int64_t> out_off(U);
  for (int u = 0; u < U; ++u) out_off[u] = (int64_t)n_best * off[u];
  HIPCHK(hipMemcpyAsync(h->nb_off.p, out_off.data(), (size_t)U * 8, hipMemcpyHostToDevice, h->stream));
  for (const uis_handle::NbestGroup& g : groups) {
    if (g.st.U < 1) continue;
    const int64_t* g_off = h->nb_off.as<int64_t>() + g.u0;
    float* g_scores = h->nb_scores.as<float>() + (size_t)g.u0 * n_best;
    int32_t* g_counts = h->nb_counts.as<int32_t>() + g.u0;
    if (!wnd)
      hipLaunchKernelGGL(k_nbest, dim3(g.st.U), dim3(UIS_NBEST_THREADS), nbest_lds_bytes(B), h->stream, g.st, (int)n_best,
                         g_off, h->nb_labels.as<int32_t>(), g_scores, g_counts,
                         stable_out ? h->nb_stable.as<long long>() + g.u0 : nullptr);
    else
      hipLaunchKernelGGL(k_nbest_window, dim3((unsigned)(((int64_t)g.st.U * n_best + 63) / 64)), dim3(64), 0, h->stream, g.st,
                         (int)n_best, g_off, h->nb_labels.as<int32_t>(), g_scores, g_counts);
    HIPCHK(hipGetLastError());
  }
  if (F > 0) HIPCHK(hipMemcpyAsync(labels_out, h->nb_labels.p, (size_t)n_best * F * 4, hipMemcpyDeviceToHost, h->stream));
  if (scores_out) HIPCHK(hipMemcpyAsync(scores_out, h->nb_scores.p, (size_t)U * n_best * 4, hipMemcpyDeviceToHost, h->stream));
  if (counts_out) HIPCHK(hipMemcpyAsync(counts_out, h->nb_counts.p, (size_t)U * 4, hipMemcpyDeviceToHost, h->stream));
  if (stable_out) HIPCHK(hipMemcpyAsync(stable_out, h->nb_stable.p, (size_t)U * 8, hipMemcpyDeviceToHost, h->stream));
  if ((rc = download_overflow(h, groups, U, overflow))) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  return UIS_OK;
}

}  // namespace

UIS_EXPORT int32_t uis_last_decode_nbest(uis_handle* h, int32_t n_best, int32_t* labels_out, int64_t capacity,
                                         float* scores_out, int32_t* counts_out) {
  if (!h) return fail(UIS_ERR_INVALID_ARG, "null handle");
  if (h->stream_state.active) return fail(UIS_ERR_INVALID_ARG, "a streaming session is open on this handle (uis_stream_nbest reads it)");
  if (!h->nb_valid)
    return fail(UIS_ERR_INVALID_ARG, "no decode on this handle that returned UIS_OK or UIS_ERR_CLUSTER_CAP");
  HIPCHK(hipSetDevice(h->device));
  return nbest_run(h, h->nb_groups, h->nb_wnd, h->nb_B, h->nb_offsets, n_best, labels_out, capacity, scores_out, counts_out,
                   nullptr, nullptr);
}

UIS_EXPORT int32_t uis_stream_nbest(uis_handle* h, int32_t n_best, int32_t* labels_out, int64_t capacity,
                                    float* scores_out, int32_t* counts_out, int64_t* stable_out) {
  if (int rc = begin_call(h, "uis_stream_nbest", UIS_RULE_STREAM_OTHER)) return rc;
  if (!session_of(h)) return UIS_ERR_INVALID_ARG;
  uis_handle::Stream& ss = h->stream_state;
  if (n_best < 1 || n_best > ss.B)
    return fail(UIS_ERR_INVALID_ARG, "n_best must be in [1, beam_size = " + std::to_string(ss.B) + "]");
  const std::vector<int64_t> off = window_offsets(ss);
  if (capacity < (int64_t)n_best * off[ss.U])
    return fail(UIS_ERR_INVALID_ARG, "labels_out: " + std::to_string((long long)n_best * off[ss.U]) + " int32 slots needed");
  std::vector<int64_t> stable_tmp;
  if (!stable_out) { stable_tmp.assign(ss.U, 0); stable_out = stable_tmp.data(); }
  return session_readout(h, [&](const std::vector<uis_handle::NbestGroup>& groups, std::vector<int32_t>* overflow) {
    if (int rc = nbest_run(h, groups, false, ss.B, off, n_best, labels_out, capacity, scores_out, counts_out, stable_out, overflow))
      return rc;
    emptied_windows(ss, counts_out, scores_out, (size_t)n_best, nullptr, 0, stable_out);  // (no labels left to show)
    return (int)UIS_OK;
  });
}
