// uis_posterior.hip -- posterior readout: per-frame confidence and speaker-turn posterior from the final beam.
//
// Per utterance, over the `live` hypotheses the n-best readout reports for the whole beam (scores s_0 <= s_1 <= ...,
// labels lab_k[t] over the N frames of the readout):
//   w_k           = exp(-(s_k - s_0) / temperature) / Z,  Z = sum_j exp(-(s_j - s_0) / temperature)
//   confidence[t] = sum_k w_k [lab_k[t] == lab_0[t]]       the beam's posterior mass behind the label predict returns
//   change[t]     = sum_k w_k [lab_k[t] != lab_k[t - 1]]   (t >= 1; change[0] = 0: the readout's first frame has no
//                                                          predecessor in the readout)
// Like the n-best readout it only reads what a decode or a session left behind; no decode kernel is involved.
//
//   k_posterior         look_ahead 1 records (DecodeState::bp, B <= 256), one workgroup per utterance, plain launch:
//                         0. the weights: e_k in float64 into LDS, Z by every wave for itself (each lane its ranks
//                            lane, lane + 64 ..., then a butterfly over the lanes), w_k = (float)(e_k / Z);
//                         1., 2. k_nbest's segment maps and stitch (nbest_segment_maps / nbest_stitch);
//                         3. a work item per (segment, group of 8 hypotheses): the 8 chains in lock-step beside rank 0's
//                            chain of that segment, each chain keeping its previous label, one record read below the
//                            segment for `change` at the segment's lowest step.  No [B][N] label table exists anywhere:
//                            an item adds its 8 terms per frame, k ascending, into its own row of a [2][groups][N]
//                            float scratch;
//                         4. a thread per frame adds the groups' rows, g ascending, in float64.
//                       k_nbest's rules to the letter: the same beam_view() and record decode (uis_beam_view.h).
//   k_posterior_window  window records (bp16: look_ahead >= 2, beams over 256), not the hot path: k_nbest_window writes
//                       the labels of every rank into a scratch table, then one workgroup per utterance forms the
//                       weights and a thread per frame sums k ascending.
// Every sum has ONE order and there are no floating-point atomics: two calls on the same state return the same bits.
// With live == 1 the one weight is exp(0) / exp(0) = 1.0f, so confidence is exactly 1.0f and change exactly 0 or 1.
//
// #included by uis_decoder.hip after uis_nbest.hip.

namespace {

#define UIS_POST_CHAINS 8   // hypotheses per work item of phase 3 (k_nbest's 8 chains in flight)

// the unnormalised weight e_k of a hypothesis at score s beside the best one's s0 (e_0 = exp(0) = 1 exactly)
__device__ __forceinline__ double posterior_e(float s, float s0, double temperature) {
  return exp(-((double)s - (double)s0) / temperature);
}

__global__ __launch_bounds__(UIS_NBEST_THREADS) void k_posterior(DecodeState st, double temperature,
                                                                 const int64_t* __restrict__ frame_off, float* __restrict__ conf,
                                                                 float* __restrict__ change, float* part,
                                                                 float* __restrict__ weights, int32_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ps_lds[];  // (NbestLds, then [B] float64 e_k, [B] float32 w_k)
  const int u = blockIdx.x;
  if (u >= st.U) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int B = st.B;
  const NbestLds lds = nbest_lds(ps_lds, B);
  unsigned char *bt_map = lds.bt_map, *ent = lds.ent;
  double* ek = reinterpret_cast<double*>(lds.more);
  float* w = reinterpret_cast<float*>(ek + B);
  const auto [N, T, par, nb, live, e, bp] = beam_view(st, u);
  const int64_t o = frame_off[u];
  if (counts && tid == 0) counts[u] = live;
  // ---- 0. the weights
  const float s0 = live > 0 ? st.beam_score[e] : 0.0f;
  for (int k = tid; k < B; k += UIS_NBEST_THREADS) ek[k] = k < live ? posterior_e(st.beam_score[e + k], s0, temperature) : 0.0;
  __syncthreads();
  double z = 0.0;
  for (int k = lane; k < B; k += 64) z += ek[k];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) z += __shfl_xor(z, m);  // (a + b on one lane, b + a on the other: the same bits)
  for (int k = tid; k < B; k += UIS_NBEST_THREADS) {
    const float wk = live > 0 ? (float)(ek[k] / z) : 0.0f;
    w[k] = wk;
    if (weights) weights[(size_t)u * B + k] = wk;
  }
  const bool walk = N > 0 && live > 0;
  if (!walk) {
    for (long t = tid; t < N; t += UIS_NBEST_THREADS) { conf[o + t] = 0.0f; change[o + t] = 0.0f; }
    return;  // (the whole workgroup)
  }
  const SegGeom sg = seg_geom(T, N);
  const int nseg = sg.nseg;
  // ---- 1. the segment maps, 2. the stitch (k_nbest's)
  nbest_segment_maps(bp, B, sg, bt_map);
  __syncthreads();
  nbest_stitch(B, live, nseg, bt_map, ent);
  __syncthreads();
  // ---- 3. item p = (segment p / groups, group p % groups) -- neighbours read the same records' rows
  const int groups = (live + UIS_POST_CHAINS - 1) / UIS_POST_CHAINS;
  float* pc = part + (size_t)2 * ((B + UIS_POST_CHAINS - 1) / UIS_POST_CHAINS) * o;  // [groups][N] confidence, then change
  float* ph = pc + (size_t)groups * N;
  for (int p = tid; p < nseg * groups; p += UIS_NBEST_THREADS) {
    const int l = p / groups, g = p - l * groups;
    const long h2 = sg.hi(l), l2 = sg.lo(l);
    int r0 = ent[l];
    int r[UIS_POST_CHAINS], prev[UIS_POST_CHAINS];
    float wk[UIS_POST_CHAINS];
#pragma unroll
    for (int k = 0; k < UIS_POST_CHAINS; ++k) {
      const int kk = g * UIS_POST_CHAINS + k;
      r[k] = kk < live ? ent[(size_t)kk * 64 + l] : r0;  // (past the live ones: rank 0's chain again at weight 0)
      wk[k] = kk < live ? w[kk] : 0.0f;
      prev[k] = 0;
    }
    float* crow = pc + (size_t)g * N;
    float* hrow = ph + (size_t)g * N;
    const long f0 = T - N;  // the step of the readout's first frame
    for (long s2 = h2; s2 >= l2; --s2) {
      const uint32_t v0 = bp[(size_t)s2 * B + r0];
      const int lab0 = rec_label(v0);
      r0 = rec_parent(v0, B);
      float c = 0.0f, ch = 0.0f;
#pragma unroll
      for (int k = 0; k < UIS_POST_CHAINS; ++k) {
        const uint32_t v = bp[(size_t)s2 * B + r[k]];
        const int lab = rec_label(v);
        r[k] = rec_parent(v, B);
        c += lab == lab0 ? wk[k] : 0.0f;
        ch += prev[k] != lab ? wk[k] : 0.0f;  // the turn between steps s2 and s2 + 1 (not stored at s2 == h2)
        prev[k] = lab;
      }
      crow[s2 - f0] = c;
      if (s2 < h2) hrow[s2 + 1 - f0] = ch;
    }
    // the turn into the segment's lowest step: one record below the segment; none below the readout's first frame
    float ch = 0.0f;
    if (l2 > f0) {
#pragma unroll
      for (int k = 0; k < UIS_POST_CHAINS; ++k) {
        const int lab = rec_label(bp[(size_t)(l2 - 1) * B + r[k]]);
        ch += prev[k] != lab ? wk[k] : 0.0f;
      }
    }
    hrow[l2 - f0] = ch;
  }
  __threadfence_block();
  __syncthreads();
  // ---- 4. the groups' rows, g ascending
  for (long t = tid; t < N; t += UIS_NBEST_THREADS) {
    double c = 0.0, ch = 0.0;
    for (int g = 0; g < groups; ++g) {
      c += (double)pc[(size_t)g * N + t];
      ch += (double)ph[(size_t)g * N + t];
    }
    conf[o + t] = fminf((float)c, 1.0f);
    change[o + t] = fminf((float)ch, 1.0f);
  }
}

// the window records: `labels` is k_nbest_window's table at n = B (utterance u at B * frame_off[u], [B][N]), scores and
// live its scores and counts
__global__ __launch_bounds__(UIS_NBEST_THREADS) void k_posterior_window(DecodeState st, double temperature,
                                                                        const int64_t* __restrict__ frame_off,
                                                                        const int32_t* __restrict__ labels,
                                                                        const float* __restrict__ scores,
                                                                        const int32_t* __restrict__ live_of,
                                                                        float* __restrict__ conf, float* __restrict__ change,
                                                                        float* weights) {
  __shared__ double zs[UIS_NBEST_THREADS];
  const int u = blockIdx.x;
  if (u >= st.U) return;
  const int tid = threadIdx.x;
  const int B = st.B;
  const long N = (long)(st.off[u + 1] - st.off[u]);
  const int live = live_of[u];
  const int64_t o = frame_off[u];
  const float* sc = scores + (size_t)u * B;
  float* w = weights + (size_t)u * B;
  const float s0 = live > 0 ? sc[0] : 0.0f;
  double z = 0.0;
  for (int k = tid; k < live; k += UIS_NBEST_THREADS) z += posterior_e(sc[k], s0, temperature);
  zs[tid] = z;
  __syncthreads();
  for (int m = UIS_NBEST_THREADS / 2; m >= 1; m >>= 1) {
    if (tid < m) zs[tid] += zs[tid + m];
    __syncthreads();
  }
  z = zs[0];
  for (int k = tid; k < B; k += UIS_NBEST_THREADS) w[k] = k < live ? (float)(posterior_e(sc[k], s0, temperature) / z) : 0.0f;
  __threadfence_block();
  __syncthreads();
  const int32_t* lab = labels + (size_t)B * o;
  for (long t = tid; t < N; t += UIS_NBEST_THREADS) {
    double c = 0.0, ch = 0.0;
    for (int k = 0; k < live; ++k) {
      const int32_t a = lab[(size_t)k * N + t];
      c += a == lab[t] ? (double)w[k] : 0.0;
      if (t > 0) ch += a != lab[(size_t)k * N + t - 1] ? (double)w[k] : 0.0;
    }
    conf[o + t] = fminf((float)c, 1.0f);
    change[o + t] = fminf((float)ch, 1.0f);
  }
}

// The readout of `groups` into the handle's ps_* buffers and on to the caller.  off: [U + 1] frame offsets.
int posterior_run(uis_handle* h, const std::vector<uis_handle::NbestGroup>& groups, bool wnd, int B, const std::vector<int64_t>& off,
                  double temperature, float* confidence_out, float* change_out, int64_t capacity, float* weights_out,
                  int32_t* counts_out, std::vector<int32_t>* overflow) {
  const int U = (int)off.size() - 1;
  if (!(temperature > 0.0) || !std::isfinite(temperature)) return fail(UIS_ERR_INVALID_ARG, "temperature must be finite and > 0");
  const int64_t F = U > 0 ? off[U] : 0;
  if ((confidence_out || change_out) && capacity < F)
    return fail(UIS_ERR_INVALID_ARG, "confidence_out / change_out: " + std::to_string((long long)F) + " float slots needed");
  if (U == 0) return UIS_OK;
  const size_t frames = (size_t)std::max<int64_t>(F, 1);
  const size_t n_groups = (size_t)(B + UIS_POST_CHAINS - 1) / UIS_POST_CHAINS;
  int rc;
  if ((rc = h->ps_conf.ensure(frames * 4))) return rc;
  if ((rc = h->ps_change.ensure(frames * 4))) return rc;
  if ((rc = h->ps_weights.ensure((size_t)U * B * 4))) return rc;
  if ((rc = h->ps_counts.ensure((size_t)U * 4))) return rc;
  if ((rc = h->ps_off.ensure((size_t)2 * U * 8))) return rc;
  if (!wnd) {
    if ((rc = h->ps_part.ensure(2 * n_groups * frames * 4))) return rc;
  } else {
    if ((rc = h->ps_labels.ensure((size_t)B * frames * 4))) return rc;
    if ((rc = h->ps_scores.ensure((size_t)U * B * 4))) return rc;
  }
  {  // UIS_POISON_WORKSPACE: the readout's own buffers (what the decode or the session left behind is its input)
    const UisPoison poison = UisPoison::from_env();
    for (DevBuf* b : {&h->ps_conf, &h->ps_change, &h->ps_weights, &h->ps_counts, &h->ps_off, &h->ps_part, &h->ps_labels, &h->ps_scores})
      if (b->p) HIPCHK(poison.device(b->p, b->cap, h->stream));
  }
  std::vector<int64_t> tab((size_t)2 * U);  // frame offsets, then k_nbest_window's label offsets at n = B
  for (int u = 0; u < U; ++u) { tab[u] = off[u]; tab[(size_t)U + u] = (int64_t)B * off[u]; }
  HIPCHK(hipMemcpyAsync(h->ps_off.p, tab.data(), (size_t)2 * U * 8, hipMemcpyHostToDevice, h->stream));
  for (const uis_handle::NbestGroup& g : groups) {
    if (g.st.U < 1) continue;
    const int64_t* g_off = h->ps_off.as<int64_t>() + g.u0;
    float* g_weights = h->ps_weights.as<float>() + (size_t)g.u0 * B;
    int32_t* g_counts = h->ps_counts.as<int32_t>() + g.u0;
    if (!wnd) {
      hipLaunchKernelGGL(k_posterior, dim3(g.st.U), dim3(UIS_NBEST_THREADS), posterior_lds_bytes(B), h->stream, g.st,
                         temperature, g_off, h->ps_conf.as<float>(), h->ps_change.as<float>(), h->ps_part.as<float>(), g_weights,
                         g_counts);
    } else {
      float* g_scores = h->ps_scores.as<float>() + (size_t)g.u0 * B;
      hipLaunchKernelGGL(k_nbest_window, dim3((unsigned)(((int64_t)g.st.U * B + 63) / 64)), dim3(64), 0, h->stream, g.st, B,
                         g_off + U, h->ps_labels.as<int32_t>(), g_scores, g_counts);
      HIPCHK(hipGetLastError());
      hipLaunchKernelGGL(k_posterior_window, dim3(g.st.U), dim3(UIS_NBEST_THREADS), 0, h->stream, g.st, temperature, g_off,
                         h->ps_labels.as<int32_t>(), g_scores, g_counts, h->ps_conf.as<float>(), h->ps_change.as<float>(), g_weights);
    }
    HIPCHK(hipGetLastError());
  }
  if (F > 0 && confidence_out) HIPCHK(hipMemcpyAsync(confidence_out, h->ps_conf.p, (size_t)F * 4, hipMemcpyDeviceToHost, h->stream));
  if (F > 0 && change_out) HIPCHK(hipMemcpyAsync(change_out, h->ps_change.p, (size_t)F * 4, hipMemcpyDeviceToHost, h->stream));
  if (weights_out) HIPCHK(hipMemcpyAsync(weights_out, h->ps_weights.p, (size_t)U * B * 4, hipMemcpyDeviceToHost, h->stream));
  if (counts_out) HIPCHK(hipMemcpyAsync(counts_out, h->ps_counts.p, (size_t)U * 4, hipMemcpyDeviceToHost, h->stream));
  if ((rc = download_overflow(h, groups, U, overflow))) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  return UIS_OK;
}

}  // namespace

UIS_EXPORT int32_t uis_last_decode_posterior(uis_handle* h, double temperature, float* confidence_out, float* change_out,
                                             int64_t capacity, float* weights_out, int32_t* counts_out) {
  if (!h) return fail(UIS_ERR_INVALID_ARG, "null handle");
  if (h->stream_state.active) return fail(UIS_ERR_INVALID_ARG, "a streaming session is open on this handle (uis_stream_posterior reads it)");
  if (!h->nb_valid)
    return fail(UIS_ERR_INVALID_ARG, "no decode on this handle that returned UIS_OK or UIS_ERR_CLUSTER_CAP");
  HIPCHK(hipSetDevice(h->device));
  return posterior_run(h, h->nb_groups, h->nb_wnd, h->nb_B, h->nb_offsets, temperature, confidence_out, change_out, capacity,
                       weights_out, counts_out, nullptr);
}

UIS_EXPORT int32_t uis_stream_posterior(uis_handle* h, double temperature, float* confidence_out, float* change_out,
                                        int64_t capacity, float* weights_out, int32_t* counts_out) {
  if (int rc = begin_call(h, "uis_stream_posterior", UIS_RULE_STREAM_OTHER)) return rc;
  if (!session_of(h)) return UIS_ERR_INVALID_ARG;
  uis_handle::Stream& ss = h->stream_state;
  if (!(temperature > 0.0) || !std::isfinite(temperature)) return fail(UIS_ERR_INVALID_ARG, "temperature must be finite and > 0");
  const std::vector<int64_t> off = window_offsets(ss);
  if ((confidence_out || change_out) && capacity < off[ss.U])
    return fail(UIS_ERR_INVALID_ARG, "confidence_out / change_out: " + std::to_string((long long)off[ss.U]) + " float slots needed");
  return session_readout(h, [&](const std::vector<uis_handle::NbestGroup>& groups, std::vector<int32_t>* overflow) {
    if (int rc = posterior_run(h, groups, false, ss.B, off, temperature, confidence_out, change_out, capacity, weights_out,
                               counts_out, overflow))
      return rc;
    const float one = 1.0f;
    emptied_windows(ss, counts_out, weights_out, (size_t)ss.B, &one);  // (no frames left to show)
    return (int)UIS_OK;
  });
}
