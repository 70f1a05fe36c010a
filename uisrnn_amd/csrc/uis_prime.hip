// uis_prime.hip -- uis_stream_prime: start the online decode of a session's utterances from a LABELED PREFIX.
//
// UIS-RNN is a generative online model: the state after a given prefix c_0 .. c_{P-1} is what _update_beam_state
// (uisrnn/uisrnn.py:388-453) leaves along that trace, and the beam search goes on from a beam that holds this one
// hypothesis.  Two halves that were already here do the work:
//   the forced run   score_run in PRIME mode (uis_score.hip): the per-cluster GRU chains of the prefix, every chain to
//                    its END -- the canonical arithmetic of uis_numerics.h, so each chain's final hidden states and
//                    running mean, and the prefix's NLL, carry the bits a decode of the same frames would have formed
//   the session      its state between two pushes is a handful of plain global-memory tables (DecodeState): the slot
//                    pool (pool_mean / pool_hid / pool_cnt), the beam tables of the parity of the utterance's step
//                    count (beam_n, beam_K / _last / _sum / _score, beam_slot / _blk), the back-pointer records bp,
//                    utt_step and overflow
// and the bridge between them is k_prime_commit + k_prime_bp below: "hypothesis 0 after P steps" written into those
// tables.  No decode kernel changes and none runs here.
//
// What a push reads again at its start, checked against the kernels: k_select / select_fast_body / the window-less
// select of enqueue_steps fetch utt_step, beam_n and the beam tables of parity utt_step & 1, pool_cnt of the live slots
// and the live slots' means at every step; the dense kernels read pool_hid / pool_mean of the rows' source slots;
// k_decode_resident (and its PERSIST launch) fetches the same tables at the first step of a launch (`fresh`), every
// slot's pool_cnt included, and writes them back when it leaves; the free slots are found from the live flags at
// every step (no free list persists); nrows / rows / gi_up / a1 / the control words are rebuilt by every push.
// k_backtrace and k_nbest read bp (rank 0's records are the only ones a walk from a live hypothesis can reach below
// step P: the beam at step P has one member), beam_n and beam_score of parity (frames received) & 1 and overflow.
// So the tables above ARE the state: nothing else persists between pushes.
//
// Layout notes.  sc_hid / sc_mean rows are in DevModel's padded layout: Hp floats per layer with the model's hidden
// units where HidMap puts them (the scoring kernels run on the same tiled weights as the decode), Dp floats per mean
// with zeros past D.  pool_hid [U][S][depth][Hp] and pool_mean [U][S][Dp] are the same layout: rows are copied, never
// re-mapped.  pool_cnt holds the frames a cluster has absorbed (k_select: nprev + 1 per row emitted; the mean update
// of the NEXT frame is uis_mean_update(M, m, nprev) with nprev = that count, which for a count of 1 drops M -- the
// reference's quirk, uisrnn.py:425-429 -- exactly as k_score_mean_scan's `p`): a chain of `len` frames stores len.
// Cluster k of the hypothesis sits in slot k of the utterance's pool (S = B * Kmax + B >= Kmax slots).
//
// The order is the scaffold's (uis_stream.hip); this call's own: between leaving the resident launch and the scratch
// come the forced run and the check of its NLLs, before anything is committed.  The launch has to leave BEFORE the
// forced run -- it occupies every CU -- so a call refused after that point (a non-finite NLL, UIS_ERR_OOM) changes no
// table but has cost the resident launch; a call refused by the host checks has not.
//
// #included by uis_decoder.hip after uis_stream.hip (the scaffold) and uis_score.hip (score_run).

namespace {

struct PrimeChain {  // one (utterance, cluster) chain of the prefix
  int64_t row;       // its last frame-row in sc_hid / sc_mean
  int32_t utt, slot, len, pad;
};

struct PrimeUtt {    // one utterance with a prefix
  int32_t utt, P, K, last, sum, blk0;  // blk0: where its clusters' block counts start in `blk`
};

struct PrimeArgs {
  int nch, nutt;
  long Fv;
  const PrimeChain* chains;   // [nch]
  const PrimeUtt* utts;       // [nutt]
  const int32_t* blk;         // block counts, (utterance, cluster) order
  const int32_t* labels;      // [F] the packed prefix labels
  const int64_t* lab_off;     // [U + 1] their offsets
  const float* hid;           // sc_hid  [depth][Fv][Hp]
  const float* mean;          // sc_mean [Fv][Dp]
  const float* scores;        // sc_out  [U]
};

// Workgroups [0, nch): chain -> slot `slot` of its utterance's pool (mean, every layer's hidden state, frame count).
// Workgroups from nch on: one thread per primed utterance writes rank 0 of the beam tables of parity P & 1, beam_n of
// both parities, utt_step and overflow.
__global__ __launch_bounds__(256) void k_prime_commit(DevModel m, DecodeState st, PrimeArgs a) {
  const int t = threadIdx.x;
  if ((int)blockIdx.x < a.nch) {
    const PrimeChain c = a.chains[blockIdx.x];
    const size_t slot = (size_t)c.utt * st.S + c.slot;
    const f32x4* src = reinterpret_cast<const f32x4*>(a.mean + (size_t)c.row * m.Dp);
    f32x4* dst = reinterpret_cast<f32x4*>(st.pool_mean + slot * m.Dp);
    for (int i = t; i < m.Dp / 4; i += 256) dst[i] = src[i];
    for (int l = 0; l < m.depth; ++l) {
      const f32x4* hs = reinterpret_cast<const f32x4*>(a.hid + ((size_t)l * a.Fv + c.row) * m.Hp);
      f32x4* hd = reinterpret_cast<f32x4*>(st.pool_hid + (slot * m.depth + l) * m.Hp);
      for (int i = t; i < m.Hp / 4; i += 256) hd[i] = hs[i];
    }
    if (t == 0) st.pool_cnt[slot] = c.len;
    return;
  }
  const int i = ((int)blockIdx.x - a.nch) * 256 + t;
  if (i >= a.nutt) return;
  const PrimeUtt p = a.utts[i];
  const int u = p.utt, par = p.P & 1;
  const size_t e = ((size_t)par * st.U + u) * st.B;
  st.beam_K[e] = p.K;
  st.beam_last[e] = p.last;
  st.beam_sum[e] = p.sum;
  st.beam_score[e] = a.scores[u];
  for (int k = 0; k < p.K; ++k) {
    st.beam_slot[e * st.Kmax + k] = k;
    st.beam_blk[e * st.Kmax + k] = a.blk[p.blk0 + k];
  }
  st.beam_n[(size_t)par * st.U + u] = 1;
  st.beam_n[(size_t)(par ^ 1) * st.U + u] = 0;
  st.utt_step[u] = p.P;
  st.overflow[u] = 0;
}

// bp records of steps 0 .. P - 1, rank 0: parent 0, cluster c_t.  One workgroup per primed utterance.
__global__ __launch_bounds__(256) void k_prime_bp(DecodeState st, PrimeArgs a) {
  const PrimeUtt p = a.utts[blockIdx.x];
  const int32_t* lab = a.labels + a.lab_off[p.utt];
  uint32_t* bp = st.bp + (size_t)st.tau * st.off[p.utt] * st.B;
  for (int s = threadIdx.x; s < p.P; s += 256) bp[(size_t)s * st.B] = (uint32_t)lab[s];
}

}  // namespace

UIS_EXPORT int32_t uis_stream_prime(uis_handle* h, const float* frames, const int64_t* offsets, const int32_t* labels,
                                    float* scores_out) {
  if (int rc = begin_call(h, "uis_stream_prime", UIS_RULE_STREAM_PRIME)) return rc;  // (the prefix's tags, in this call's frame order)
  if (!session_of(h, offsets != nullptr, "null handle/offsets")) return UIS_ERR_INVALID_ARG;
  uis_handle::Stream& ss = h->stream_state;
  const DevModel& m = h->m;
  const int U = ss.U;
  CallTimer timer{h};
  // ---- the checks
  if (offsets[0] != 0) return fail(UIS_ERR_INVALID_ARG, "offsets[0] must be 0");
  for (int u = 0; u < U; ++u)
    if (offsets[u + 1] < offsets[u]) return fail(UIS_ERR_INVALID_ARG, "offsets must be non-decreasing");
  const int64_t F = offsets[U];
  if (F > 0 && (!frames || !labels)) return fail(UIS_ERR_INVALID_ARG, "frames/labels is null");
  if (F > 0x7fffffffLL) return fail(UIS_ERR_UNSUPPORTED, "more than 2^31 - 1 frames in one call");
  if (int rct = table_status(h->tables.check_stream_tags("call", F))) return rct;
  if (h->tables.stream_tags.call_set && (ss.st.flags & UIS_FLAG_PERSISTENT))  // (its pushes could never name the tags again)
    return fail(UIS_ERR_UNSUPPORTED, "a UIS_FLAG_PERSISTENT session takes no known speakers (uis_stream_speakers): the table is dropped");
  const uint8_t* tags = h->tables.stream_tags.data();
  int too_many = -1, too_many_K = 0;
  std::vector<std::vector<uint8_t>> tag_of_label(U);
  for (int u = 0; u < U; ++u) {
    const int64_t P = offsets[u + 1] - offsets[u];
    if (P == 0) continue;
    if (ss.committed[u] + ss.have[u] != 0)  // (an utterance whose window is empty after a commit has received frames all the same)
      return fail(UIS_ERR_INVALID_ARG, "utterance " + std::to_string(u) + " has already received or been primed with " +
                                           std::to_string((long long)(ss.committed[u] + ss.have[u])) + " frames: a prefix goes in front of everything");
    if (P > ss.cap) return fail(UIS_ERR_INVALID_ARG, "utterance " + std::to_string(u) + ": the prefix exceeds the session's max_frames");
    if (int rct = table_status(CallTables::check_tagged_frames("uis_stream_prime", ss.tagged || h->tables.tagged, u, P))) return rct;
    int K = 0;
    // (the binding hypothesis 0 would hold after these labels under these tags: tag_of_label[u][c], 0 = none; the decode's
    // rule admits the trace iff tag <-> label is a partial bijection)
    std::vector<uint8_t>& tag_of = tag_of_label[u];
    int label_of[128];
    std::fill(label_of, label_of + 128, -1);
    for (int64_t t = offsets[u]; t < offsets[u + 1]; ++t) {
      const int c = labels[t];
      if (c < 0) return fail(UIS_ERR_INVALID_ARG, "label " + std::to_string(c) + " at frame " + std::to_string(t) + " is negative");
      if (c > K)
        return fail(UIS_ERR_INVALID_ARG, "label " + std::to_string(c) + " at frame " + std::to_string(t) +
                                             " is not in first-appearance form (at most " + std::to_string(K) + " here): a prefix "
                                             "cannot be an invalid trace");
      if (c == K) { ++K; tag_of.push_back(0); }
      const int g = tags ? tags[t] : 0;
      if (!g) continue;
      if ((tag_of[c] && tag_of[c] != g) || (label_of[g] >= 0 && label_of[g] != c))
        return fail(UIS_ERR_INVALID_ARG, "utterance " + std::to_string(u) + ": the prefix labels contradict its tags (tag " + std::to_string(g) +
                                             " on label " + std::to_string(c) + " at frame " + std::to_string(t) + ")");
      tag_of[c] = (uint8_t)g;
      label_of[g] = c;
    }
    if (K > ss.Kmax && too_many < 0) { too_many = u; too_many_K = K; }
  }
  if (too_many >= 0)
    return fail(UIS_ERR_CLUSTER_CAP, "utterance " + std::to_string(too_many) + ": the prefix has " + std::to_string(too_many_K) +
                                         " clusters, the session's max_clusters is " + std::to_string(ss.Kmax));
  if (F == 0) {
    if (scores_out) std::fill(scores_out, scores_out + U, 0.0f);
    return UIS_OK;
  }
  int rc;
  if ((rc = session_enter(h, nullptr))) return rc;  // (no window table: nothing here reads one)
  // ---- the forced run: every chain to its end; the NLLs come back before anything is committed
  ScoreSchedule s;
  std::vector<float> nll(U, 0.0f);
  if ((rc = score_run(h, frames, offsets, U, labels, nll.data(), nullptr, &s))) return rc;
  for (int u = 0; u < U; ++u)
    if (offsets[u + 1] > offsets[u] && !std::isfinite(nll[u]))
      return fail(UIS_ERR_INVALID_ARG, "utterance " + std::to_string(u) + ": the prefix's negative log-likelihood is not finite");
  // ---- the commit tables
  const int nch = (int)s.len.size();
  std::vector<PrimeChain> chains(nch);
  std::vector<PrimeUtt> utts;
  for (int u = 0; u < U; ++u) {
    const int K = s.chain_base[u + 1] - s.chain_base[u];
    if (K == 0) continue;
    // (uis_session_min_turn: under a slot's m >= 2 the word carries min(trailing run of the prefix labels, m), as the
    // selects would have left it; turns shorter than m INSIDE the prefix are the caller's and are kept)
    int32_t last_word = s.utt_last[u];
    if (const int32_t mt = ss.min_turn[u]; mt >= 2) {
      int32_t run = 1;
      for (int64_t t = offsets[u + 1] - 1; t > offsets[u] && run < mt && labels[t - 1] == labels[t]; --t) ++run;
      last_word |= run << UIS_LAST_RUN_SHIFT;
    }
    utts.push_back(PrimeUtt{u, (int32_t)(offsets[u + 1] - offsets[u]), K, last_word, s.utt_sum[u], s.chain_base[u]});
    for (int k = 0; k < K; ++k) {
      const int i = s.rank[s.chain_base[u] + k], len = s.len[i];
      chains[i] = PrimeChain{s.fbase[len - 1] + i, u, k, len, 0};
    }
  }
  const int nutt = (int)utts.size();
  // (uis_stream_speakers: the binding rides in the block-count words, as the selects leave it -- count | tag << 24)
  std::vector<int32_t> blk_words(s.chain_blk.begin(), s.chain_blk.end());
  for (const PrimeUtt& p : utts)
    for (int k = 0; k < p.K; ++k) blk_words[p.blk0 + k] |= (int32_t)tag_of_label[p.utt][k] << UIS_BLK_TAG_SHIFT;
  ss.tagged = ss.tagged || h->tables.tagged;
  ScratchPlan plan;
  const size_t o_chains = plan.take((size_t)nch * sizeof(PrimeChain)), o_utts = plan.take((size_t)nutt * sizeof(PrimeUtt)),
               o_blk = plan.take((size_t)nch * 4), o_lab = plan.take((size_t)F * 4);
  char* base;
  if ((rc = session_buffers(h, plan, 0, &base))) return rc;
  hipStream_t st = h->stream;
  HIPCHK(hipMemcpyAsync(base + o_chains, chains.data(), (size_t)nch * sizeof(PrimeChain), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(base + o_utts, utts.data(), (size_t)nutt * sizeof(PrimeUtt), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(base + o_blk, blk_words.data(), (size_t)nch * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(base + o_lab, labels, (size_t)F * 4, hipMemcpyHostToDevice, st));
  PrimeArgs a{};
  a.nch = nch; a.nutt = nutt; a.Fv = (long)s.Fv;
  a.chains = reinterpret_cast<const PrimeChain*>(base + o_chains);
  a.utts = reinterpret_cast<const PrimeUtt*>(base + o_utts);
  a.blk = reinterpret_cast<const int32_t*>(base + o_blk);
  a.labels = reinterpret_cast<const int32_t*>(base + o_lab);
  a.lab_off = h->sc_utt.as<int64_t>();  // (score_run left the offsets there)
  a.hid = h->sc_hid.as<float>();
  a.mean = h->sc_mean.as<float>();
  a.scores = h->sc_out.as<float>();
  // ---- the commit
  HIPCHK(timer.begin());
  hipLaunchKernelGGL(k_prime_commit, dim3((unsigned)(nch + (nutt + 255) / 256)), dim3(256), 0, st, m, ss.st, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_prime_bp, dim3((unsigned)nutt), dim3(256), 0, st, ss.st, a);
  HIPCHK(hipGetLastError());
  HIPCHK(timer.end());
  HIPCHK(hipStreamSynchronize(st));
  for (const PrimeUtt& p : utts) ss.have[p.utt] = p.P;
  if (scores_out) std::copy(nll.begin(), nll.end(), scores_out);
  if (score_timing_env())
    fprintf(stderr, "uis_stream_prime: utterances %d chains %d commit_device_ms %.3f call_ms %.3f\n", nutt, nch, timer.device_ms(),
            timer.call_ms());
  return UIS_OK;
}
