// uis_retire.hip -- uis_stream_retire: delete clusters that no live hypothesis of a session can still name from the
// hypotheses' tables, so that an endless stream stays under max_clusters.
//
// uis_stream_commit gives back the room of old frames; the cluster tables -- K, the slot / block lists -- only ever
// grow.  Between two pushes (uis_prime.hip's header comment names the tables), with N = the frames in the window and
// the live hypotheses = ranks 0 .. live - 1 of the beam tables of parity N & 1, cluster index k is RETIRABLE iff for
// every live rank r:  k < K_r,  k is not among r's labels of window frames [0, N) (its back-pointer chain, walked as
// k_nbest walks it),  and k != last_r (a window that a commit emptied has no labels, and its one hypothesis still
// continues from its last label),  and k carries no speaker tag in r's block-count words (uis_stream_speakers: the next
// frame with that tag names it; the words move down whole, so a binding follows its cluster's new index).  Such a
// cluster was opened before the window; after a commit or a prime all live
// hypotheses share that history, so index k means the same speaker in each of them.  Retiring a set R:
//   lists    every live rank's slot / block lists lose the entries in R, the entries above move down in order
//   scalars  K_r -= |R|,  sum_r -= sum of blk_r[k] over R,  last_r -= #{k in R : k < last_r};  scores stay.  last_r is
//            the LABEL of the rank's last-label word (last_label(): a slot with a minimum turn length keeps the run in
//            bits 16 .. 30, uis_session_min_turn); the run bits stay as they are
//   records  in every record word of window steps [0, N) the label becomes label - #{k in R : k < label}; the parent
//            stays.  Words of ranks that are not live are stale (any bit pattern): a label above max_clusters is left
// and nothing else: a retired cluster's slot is free by itself (the selects find free slots from the live lists at
// every step), utt_step, the prior tables and the pool are not touched.  The ddCRP denominator sum + alpha shrinks with
// sum_r: for the prior the speaker never existed.
//
// Two kernels, one workgroup per utterance, between launches, no decode kernel, no floating point, no global atomics:
//   k_retire_scan   the used indices into an LDS bit mask (k_nbest's phases 1 and 2, then every (segment, hypothesis)
//                   pair walks its segment once), the lasts, min / max K; the selection -- every retirable index, or
//                   the caller's list, each entry checked -- as a second mask; the shift table [Kmax + 1]
//                   (shift[k] = selected indices below k), the retired and the retirable lists, the counts, and a
//                   status word: 1 = the list names an index that is not retirable
//   k_retire_apply  leaves at once if ANY utterance's status is set (a refusal changes no bit of the session); else
//                   the scalars, then the lists (in place, source and destination overlap: read, barrier, write, as
//                   k_commit_prune), then the window's N * B record words, 16 bytes per thread where the utterance's
//                   records are aligned, a scalar tail, and the scalar path where they are not
// An utterance with an emptied beam or flagged in the overflow word has live = 0: nothing is retirable, it is left
// alone; one that has received nothing holds the empty hypothesis (K = 0): likewise.
//
// The order is the scaffold's (uis_stream.hip); this call's own: the refusal of a selection is found on the device and
// reported after the download, with no bit of the session changed.
//
// #included by uis_decoder.hip after uis_nbest.hip (nbest_segment_maps, nbest_stitch) and uis_restart.hip.

namespace {

#define UIS_RETIRE_THREADS 256
#define UIS_RETIRE_MASK_WORDS 129   // bits 0 .. 4096 (max_clusters <= 4096, and the table's entry Kmax)
#define UIS_RETIRE_QUERY 0          // per-utterance modes
#define UIS_RETIRE_ALL 1
#define UIS_RETIRE_LIST 2

struct RetireArgs {
  const int32_t* mode;      // [U]
  const int64_t* sel_off;   // [U + 1] (UIS_RETIRE_LIST)
  const int32_t* sel;       // the packed lists, each ascending and within [0, Kmax): the host has checked that
  int32_t* shift;           // [U][Kmax + 1]
  int32_t* retired;         // [U][Kmax]
  int32_t* retirable;       // [U][Kmax]
  int32_t* words;           // [U][4]: retired, retirable, largest K afterwards, status
  int tagged;               // the session holds speaker tags (uis_stream_speakers): the block-count words are scanned for them
};

// pre[w] = bits set in mask[0 .. w), w <= nw (one thread; nw <= 129)
__device__ __forceinline__ void retire_prefix(const uint32_t* mask, int* pre, int nw) {
  int acc = 0;
  for (int w = 0; w < nw; ++w) { pre[w] = acc; acc += __popc(mask[w]); }
  pre[nw] = acc;
}

__device__ __forceinline__ int retire_below(const uint32_t* mask, const int* pre, int k) {
  return pre[k >> 5] + __popc(mask[k >> 5] & ((1u << (k & 31)) - 1u));
}

__global__ __launch_bounds__(UIS_RETIRE_THREADS) void k_retire_scan(DecodeState st, RetireArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rt_lds[];  // (NbestLds)
  __shared__ uint32_t s_used[UIS_RETIRE_MASK_WORDS], s_sel[UIS_RETIRE_MASK_WORDS], s_able[UIS_RETIRE_MASK_WORDS];
  __shared__ int s_pre_sel[UIS_RETIRE_MASK_WORDS + 1], s_pre_able[UIS_RETIRE_MASK_WORDS + 1];
  __shared__ int s_minK, s_maxK, s_bad;
  const int u = blockIdx.x, tid = threadIdx.x;
  if (u >= st.U) return;
  const int B = st.B, Kmax = st.Kmax;
  const int nw = (Kmax >> 5) + 1;   // words that hold bits 0 .. Kmax
  const NbestLds lds = nbest_lds(rt_lds, B);
  unsigned char *bt_map = lds.bt_map, *ent = lds.ent;
  const auto [N, T, par, nb, live, e, bp] = beam_view(st, u, EMPTY_WINDOW_KEEPS_BEAM);
  for (int w = tid; w < UIS_RETIRE_MASK_WORDS; w += UIS_RETIRE_THREADS) { s_used[w] = 0; s_sel[w] = 0; s_able[w] = 0; }
  if (tid == 0) { s_minK = Kmax; s_maxK = 0; s_bad = 0; }
  const bool walk = N > 0 && live > 0;
  const SegGeom g = seg_geom(N, N);
  const int nseg = g.nseg;
  // ---- the chains of the live ranks over the window (k_nbest's phases 1 and 2)
  if (walk) nbest_segment_maps(bp, B, g, bt_map);
  __syncthreads();
  if (walk) nbest_stitch(B, live, nseg, bt_map, ent);
  __syncthreads();
  // ---- the used indices: pair p = (segment p / live, hypothesis p % live)
  if (walk) {
    for (int p = tid; p < nseg * live; p += UIS_RETIRE_THREADS) {
      const int l = p / live, k = p - l * live;
      walk_segment(bp, B, g, l, ent[(size_t)k * 64 + l], [&](long, uint32_t v) {
        const int lab = rec_label(v);
        if (lab < Kmax) atomicOr(&s_used[lab >> 5], 1u << (lab & 31));   // (LDS)
      });
    }
  }
  // ---- the lasts count as used; min and max K over the live ranks
  for (int r = tid; r < live; r += UIS_RETIRE_THREADS) {
    int K = st.beam_K[e + r];
    K = K < 0 ? 0 : (K > Kmax ? Kmax : K);
    const int last = last_label(st.beam_last[e + r]);   // (the label, whatever run the word carries: uis_session_min_turn)
    if (last >= 0 && last < Kmax) atomicOr(&s_used[last >> 5], 1u << (last & 31));
    atomicMin(&s_minK, K);
    atomicMax(&s_maxK, K);
  }
  // ---- a cluster that carries a tag in any live rank counts as used: the next frame with that tag names it.  Entry
  // i = (rank i / Kmax, index i % Kmax)
  if (a.tagged) {
    for (long i = tid; i < (long)live * Kmax; i += UIS_RETIRE_THREADS) {
      const int r = (int)(i / Kmax), k = (int)(i - (long)r * Kmax);
      const int K = st.beam_K[e + r];
      if (k < K && blk_tag(st.beam_blk[(e + r) * Kmax + k]) != 0) atomicOr(&s_used[k >> 5], 1u << (k & 31));
    }
  }
  __syncthreads();
  const int minK = live > 0 ? s_minK : 0;
  // ---- retirable = below every K and not used
  for (int w = tid; w < nw; w += UIS_RETIRE_THREADS) {
    const int k0 = w << 5;
    uint32_t below = 0;
    if (minK >= k0 + 32) below = 0xffffffffu;
    else if (minK > k0) below = (1u << (minK - k0)) - 1u;
    s_able[w] = below & ~s_used[w];
  }
  __syncthreads();
  // ---- the selection
  const int mode = a.mode[u];
  if (mode == UIS_RETIRE_ALL) {
    for (int w = tid; w < nw; w += UIS_RETIRE_THREADS) s_sel[w] = s_able[w];
  } else if (mode == UIS_RETIRE_LIST) {
    const int64_t i0 = a.sel_off[u], i1 = a.sel_off[u + 1];
    for (int64_t i = i0 + tid; i < i1; i += UIS_RETIRE_THREADS) {
      const int k = a.sel[i];
      if (k < 0 || k >= Kmax || !((s_able[k >> 5] >> (k & 31)) & 1u)) atomicOr(&s_bad, 1);
      else atomicOr(&s_sel[k >> 5], 1u << (k & 31));
    }
  }
  __syncthreads();
  if (tid == 0) retire_prefix(s_sel, s_pre_sel, nw);
  if (tid == 64) retire_prefix(s_able, s_pre_able, nw);
  __syncthreads();
  // ---- the shift table, the two lists, the counts
  int32_t* shift = a.shift + (size_t)u * (Kmax + 1);
  int32_t* retired = a.retired + (size_t)u * Kmax;
  int32_t* retirable = a.retirable + (size_t)u * Kmax;
  for (int k = tid; k <= Kmax; k += UIS_RETIRE_THREADS) {
    const int below = retire_below(s_sel, s_pre_sel, k);
    shift[k] = below;
    if (k < Kmax) {
      if ((s_sel[k >> 5] >> (k & 31)) & 1u) retired[below] = k;
      if ((s_able[k >> 5] >> (k & 31)) & 1u) retirable[retire_below(s_able, s_pre_able, k)] = k;
    }
  }
  if (tid == 0) {
    const int n_ret = s_pre_sel[nw];
    a.words[4 * u + 0] = n_ret;
    a.words[4 * u + 1] = s_pre_able[nw];
    a.words[4 * u + 2] = live > 0 ? s_maxK - n_ret : 0;
    a.words[4 * u + 3] = s_bad;
  }
}

__global__ __launch_bounds__(UIS_RETIRE_THREADS) void k_retire_apply(DecodeState st, RetireArgs a) {
  __shared__ int s_shift[4097];
  __shared__ int s_K[256];   // (beam_size <= 256)
  const int u = blockIdx.x, tid = threadIdx.x;
  if (u >= st.U) return;
  // ---- a selection refused for any utterance: nobody writes
  int bad = 0;
  for (int v = tid; v < st.U; v += UIS_RETIRE_THREADS) bad |= a.words[4 * v + 3];
  if (__syncthreads_or(bad)) return;
  const int n_ret = a.words[4 * u + 0];
  if (n_ret <= 0) return;
  const int B = st.B, Kmax = st.Kmax;
  const auto [N, T, par, nb, live, e, bp] = beam_view(st, u, EMPTY_WINDOW_KEEPS_BEAM);   // (live > 0: nothing is retirable without a live hypothesis)
  const int32_t* shift = a.shift + (size_t)u * (Kmax + 1);
  const int32_t* retired = a.retired + (size_t)u * Kmax;
  for (int k = tid; k <= Kmax; k += UIS_RETIRE_THREADS) s_shift[k] = shift[k];
  __syncthreads();
  // ---- the scalars (the block counts are read here, before the lists move; K before the call stays in LDS)
  for (int r = tid; r < live; r += UIS_RETIRE_THREADS) {
    const int32_t* blk = st.beam_blk + (e + r) * Kmax;
    int gone = 0;
    for (int i = 0; i < n_ret; ++i) gone += blk_count(blk[retired[i]]);   // (a retired cluster carries no tag; the count all the same)
    const int K = st.beam_K[e + r], word = st.beam_last[e + r], last = last_label(word);
    s_K[r] = K < 0 ? 0 : (K > Kmax ? Kmax : K);
    st.beam_K[e + r] = K - n_ret;
    st.beam_sum[e + r] -= gone;
    // (the renumbered label under the word's unchanged run bits; a word without run bits is the label, as before)
    if (word > 0 && last > 0 && last <= Kmax) st.beam_last[e + r] = word - s_shift[last];
  }
  loads_before_stores();  // (the block counts have returned before the barrier lets anyone move them)
  // ---- the lists: entry i = (rank i / Kmax, index i % Kmax), ascending tiles.  An entry moves down inside its row,
  // into this tile or an earlier one: every tile is in registers before any of it is stored.
  const long entries = (long)live * Kmax;
  for (long base = 0; base < entries; base += UIS_RETIRE_THREADS) {
    const long i = base + tid;
    size_t row = 0;
    int dst = -1;
    int32_t vslot = 0, vblk = 0;
    if (i < entries) {
      const int r = (int)(i / Kmax), k = (int)(i - (long)r * Kmax);
      row = (e + r) * Kmax;
      if (k < s_K[r] && s_shift[k + 1] == s_shift[k]) {   // a live entry that stays
        dst = k - s_shift[k];
        vslot = st.beam_slot[row + k];
        vblk = st.beam_blk[row + k];
      }
    }
    loads_before_stores();
    if (dst >= 0) {
      st.beam_slot[row + dst] = vslot;
      st.beam_blk[row + dst] = vblk;
    }
  }
  // ---- the records of window steps [0, N): every word its own thread's, no overlap
  const long words = N * (long)B;
  auto relabel = [&](uint32_t v) {
    const uint32_t lab = (uint32_t)rec_label(v);
    return lab <= (uint32_t)Kmax ? (v & 0xffff0000u) | (lab - (uint32_t)s_shift[lab]) : v;
  };
  if ((reinterpret_cast<uintptr_t>(bp) & 15u) == 0) {
    const long nvec = words >> 2;
    uint4* b4 = reinterpret_cast<uint4*>(bp);
    for (long i = tid; i < nvec; i += UIS_RETIRE_THREADS) {
      uint4 v = b4[i];
      v.x = relabel(v.x); v.y = relabel(v.y); v.z = relabel(v.z); v.w = relabel(v.w);
      b4[i] = v;
    }
    const long i = (nvec << 2) + tid;   // the scalar tail: up to three words
    if (i < words) bp[i] = relabel(bp[i]);
  } else {
    for (long i = tid; i < words; i += UIS_RETIRE_THREADS) bp[i] = relabel(bp[i]);
  }
}

}  // namespace

UIS_EXPORT int32_t uis_stream_retire(uis_handle* h, const int32_t* which, const int64_t* offsets, const int32_t* clusters,
                                     int32_t* retired_out, int32_t* counts_out, int32_t* k_out, int32_t* retirable_out,
                                     int32_t* retirable_counts_out) {
  if (int rc = begin_call(h, "uis_stream_retire", UIS_RULE_STREAM_OTHER)) return rc;
  if (!session_of(h, counts_out && k_out, "null handle/counts_out/k_out")) return UIS_ERR_INVALID_ARG;
  uis_handle::Stream& ss = h->stream_state;
  const int U = ss.U, B = ss.B, Kmax = ss.Kmax;
  CallTimer timer{h};
  // ---- the checks
  if (clusters && !offsets) return fail(UIS_ERR_INVALID_ARG, "clusters without offsets");
  if (offsets && which) return fail(UIS_ERR_INVALID_ARG, "which and an explicit selection (offsets) exclude each other");
  std::vector<int32_t> mode(U, UIS_RETIRE_QUERY);
  int64_t n_sel = 0;
  if (offsets) {
    if (offsets[0] != 0) return fail(UIS_ERR_INVALID_ARG, "offsets[0] must be 0");
    for (int u = 0; u < U; ++u)
      if (offsets[u + 1] < offsets[u]) return fail(UIS_ERR_INVALID_ARG, "offsets must be non-decreasing");
    n_sel = offsets[U];
    if (n_sel > 0 && !clusters) return fail(UIS_ERR_INVALID_ARG, "clusters is null");
    if (n_sel > 0 && !retired_out) return fail(UIS_ERR_INVALID_ARG, "retired_out is null");
    for (int u = 0; u < U; ++u) {
      for (int64_t i = offsets[u]; i < offsets[u + 1]; ++i) {
        const int32_t k = clusters[i];
        if (k < 0 || k >= Kmax)
          return fail(UIS_ERR_INVALID_ARG, "utterance " + std::to_string(u) + ": cluster index " + std::to_string(k) +
                                               " is out of range [0, max_clusters = " + std::to_string(Kmax) + ")");
        if (i > offsets[u] && k <= clusters[i - 1])
          return fail(UIS_ERR_INVALID_ARG, "utterance " + std::to_string(u) + ": cluster indices must be ascending and distinct (" +
                                               std::to_string(clusters[i - 1]) + " before " + std::to_string(k) + ")");
      }
      if (offsets[u + 1] > offsets[u]) mode[u] = UIS_RETIRE_LIST;
    }
  } else {
    if (!retired_out) return fail(UIS_ERR_INVALID_ARG, "retired_out is null");
    for (int u = 0; u < U; ++u) mode[u] = !which || which[u] ? UIS_RETIRE_ALL : UIS_RETIRE_QUERY;
  }
  int rc;
  DecodeState stc;
  if ((rc = session_enter(h, &stc))) return rc;
  hipStream_t st = h->stream;
  // ---- scratch: [mode U][offsets U + 1][lists] go up in one copy, [words 4 U][retired U Kmax][retirable U Kmax] come
  // back in one; the shift tables stay on the device
  ScratchPlan plan;
  const size_t o_mode = plan.take((size_t)U * 4), o_off = plan.take((size_t)(U + 1) * 8), o_sel = plan.take((size_t)n_sel * 4, 4),
               o_words = plan.take((size_t)U * 16), o_ret = plan.take((size_t)U * Kmax * 4, 4),
               o_able = plan.take((size_t)U * Kmax * 4, 4), o_shift = plan.take((size_t)U * (Kmax + 1) * 4, 4),
               land = o_shift - o_words;
  char* base;
  if ((rc = session_buffers(h, plan, land, &base))) return rc;
  std::vector<char> up(o_words, 0);
  std::copy(mode.begin(), mode.end(), reinterpret_cast<int32_t*>(up.data() + o_mode));
  if (offsets) std::copy(offsets, offsets + U + 1, reinterpret_cast<int64_t*>(up.data() + o_off));
  if (n_sel > 0) std::copy(clusters, clusters + n_sel, reinterpret_cast<int32_t*>(up.data() + o_sel));
  HIPCHK(hipMemcpyAsync(base, up.data(), o_words, hipMemcpyHostToDevice, st));
  RetireArgs a{};
  a.mode = reinterpret_cast<const int32_t*>(base + o_mode);
  a.sel_off = reinterpret_cast<const int64_t*>(base + o_off);
  a.sel = reinterpret_cast<const int32_t*>(base + o_sel);
  a.words = reinterpret_cast<int32_t*>(base + o_words);
  a.retired = reinterpret_cast<int32_t*>(base + o_ret);
  a.retirable = reinterpret_cast<int32_t*>(base + o_able);
  a.shift = reinterpret_cast<int32_t*>(base + o_shift);
  a.tagged = ss.tagged ? 1 : 0;
  // ---- scan, apply
  HIPCHK(timer.begin());
  hipLaunchKernelGGL(k_retire_scan, dim3(U), dim3(UIS_RETIRE_THREADS), nbest_lds_bytes(B), st, stc, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_retire_apply, dim3(U), dim3(UIS_RETIRE_THREADS), 0, st, stc, a);
  HIPCHK(hipGetLastError());
  HIPCHK(timer.end());
  HIPCHK(hipMemcpyAsync(ss.h_land.p, base + o_words, land, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  // ---- the host's side
  const int32_t* h_words = ss.h_land.as<int32_t>();
  const int32_t* h_ret = h_words + 4 * (size_t)U;
  const int32_t* h_able = h_ret + (size_t)U * Kmax;
  for (int u = 0; u < U; ++u)
    if (h_words[4 * u + 3])
      return fail(UIS_ERR_INVALID_ARG, "utterance " + std::to_string(u) + ": the selection names a cluster that is not retirable "
                                           "(in use in the window, the last label of a live hypothesis, or not below every live K); nothing was retired");
  int64_t n_retired = 0;
  for (int u = 0; u < U; ++u) {
    const int32_t n = h_words[4 * u + 0], m = h_words[4 * u + 1];
    counts_out[u] = n;
    k_out[u] = h_words[4 * u + 2];
    if (retired_out) std::copy(h_ret + (size_t)u * Kmax, h_ret + (size_t)u * Kmax + n, retired_out + (size_t)u * Kmax);
    if (retirable_counts_out) retirable_counts_out[u] = m;
    if (retirable_out) std::copy(h_able + (size_t)u * Kmax, h_able + (size_t)u * Kmax + m, retirable_out + (size_t)u * Kmax);
    n_retired += n;
  }
  if (n_retired) h->nb_valid = false;
  if (CallTimer::env("UIS_RETIRE_TRACE"))
    fprintf(stderr, "uis_stream_retire: utterances %d window_frames %lld selected %lld retired %lld device_ms %.3f call_ms %.3f\n",
            U, (long long)window_offsets(ss)[U], offsets ? (long long)n_sel : -1ll, (long long)n_retired, timer.device_ms(), timer.call_ms());
  return UIS_OK;
}
