// uis_score.hip -- uis_score_labels: the model's negative log-likelihood of a GIVEN labeling.
//
// The neg_likelihood the beam search minimises (uisrnn/uisrnn.py:388-453, _update_beam_state) applied
// along a fixed trace c_0 .. c_{N-1} from an empty BeamState, test_iteration 1.  Once the labels are
// known each cluster's GRU chain is independent of the others, so the work is split as
//   schedule (host)  the chains (utterance, cluster), each frame's position in its chain, the float64
//                    prior of every frame (the decode's expressions and logblk / logden tables), the
//                    chains ordered longest first: the chains active at position p are a prefix
//   frame stream     k_pad_frames, k_dense_input_proj[_wide] (gi0), k_mse0 -- the decode's own kernels
//   recurrence       a launch per (position, layer): W_hh h + b_hh and the GRU unit for every chain
//                    still running (k_score_gru), layers >= 1 with their input-side gates first
//                    (k_score_upper_in); split-K MFMA tiles, the canonical order of uis_numerics.h
//   heads            linear_mean1 + relu, linear_mean2 over all rows at once (k_score_head, full-K tiles)
//   losses           the running mean per chain (k_score_mean_scan), the weighted MSE against it and
//                    the step loss per frame (k_score_loss), the float32 sum per utterance in frame
//                    order (k_score_sum)
// A frame-row r is one (chain, position) pair; rows are position-major: row(p, i) = fbase[p] + i for the
// i-th longest chain.  The GRU of a chain's last row is not run (its state is never read) -- except in PRIME mode
// (score_run's `keep`, uis_prime.hip): there every chain runs to its end, the recurrence and the mean scan cover the
// last row too, and each chain's final hidden states and running mean are what a session is primed with.  The rows a
// scoring call computes and the kernels that compute them are the same in both modes.
//
// uis_score_speakers (score_run's `spk`) runs the chains to their ends as PRIME mode does and then reads sc_mean once per
// (frame, open cluster) instead of once per frame: the whole _calculate_score row along the fixed trace, not only the
// chosen column.  Which mean row a cluster holds at a frame, its block count, and each frame's K / sum(block_counts) /
// last label are formed on the device from the labels (k_speakers_tables); the candidates are scored by
// k_score_speakers.  Nothing the other two modes launch changes.
//
// uis_speaker_profiles (score_run's `prof`) is the third mode that runs the chains to their ends:
// a chain is a cluster, and after the tail scan its last row of sc_mean is the cluster's final running mean.  One more
// kernel (k_score_profile_scan) walks every chain once more and leaves its frame count, block count, first and last
// frame, that mean, the float32 sum of its frames and the float32 sum of the squared residuals x - (the mean the frame
// was charged against), per dimension.  Which (utterance, cluster) a chain is comes from the schedule (chain_base, rank,
// chain_blk).  Nothing the plain scoring run, PRIME mode or uis_score_speakers launches changes.
//
// #included by uis_decoder.hip after the handle, Launcher and the decode kernels.

namespace {

// One launch of the recurrence: position p, layer `layer`.
struct ScoreStep {
  int n;                     // chains active at this position (a prefix of the longest-first order)
  int layer;
  long row0;                 // row(p, 0)
  long prev0;                // row(p - 1, 0), or -1 at p = 0 (the state before a cluster's first frame is h1)
  long Fv;                   // frame-rows: the stride of one layer in `hid`
  const int32_t* row_frame;  // [Fv] frame of each row in the packed stream
  const float* gi0;          // [F][G]
  float* gi_up;              // [n][G] input-side gates of `layer` >= 1
  float* hid;                // [depth][Fv][Hp]
};

__device__ __forceinline__ float* score_hid(const DevModel& m, const ScoreStep& a, int layer, long row) {
  return a.hid + ((size_t)layer * a.Fv + row) * m.Hp;
}

// gi_up[i] = b_ih + W_ih h'_{layer-1}(row(p, i))   (one 16 x 16 tile per workgroup, split-K)
__global__ __launch_bounds__(512) void k_score_upper_in(DevModel m, ScoreStep a) {
  __shared__ __attribute__((aligned(16))) float spart[UIS_KSPLIT * 256];
  const int nrt = (a.n + 15) >> 4, nft = m.G / 16;
  int rt, ft;
  dense_block_map(blockIdx.x, nrt, nft, rt, ft);
  if (rt >= nrt || ft >= nft) return;
  const int t = threadIdx.x;
  int i = rt * 16 + (t & 15);
  if (i >= a.n) i = a.n - 1;  // (rows past the count stream the last row; not stored)
  const float* in[1] = {score_hid(m, a, a.layer - 1, a.row0 + i)};
  splitk_tile<1, 1, 1>(m.wih[a.layer], 0, ft, m.Hp / 16, in, m.bih[a.layer] + ft * 16, 0, spart);
  if (t >= 256) return;
  const int er = rt * 16 + (t >> 4);
  if (er >= a.n) return;
  a.gi_up[(size_t)er * m.G + ft * 16 + (t & 15)] = splitk_combine<1, 1>(spart, 0, 0, t);
}

// h'(row(p, i)) = GRU(gi, b_hh + W_hh h(row(p - 1, i)), h(row(p - 1, i)))   (as k_dense_gru<1>)
__global__ __launch_bounds__(512) void k_score_gru(DevModel m, ScoreStep a) {
  __shared__ __attribute__((aligned(16))) float spart[UIS_KSPLIT * 3 * 256];
  const int nrt = (a.n + 15) >> 4, nft = m.Hp / 16;
  int rt, ft;
  dense_block_map(blockIdx.x, nrt, nft, rt, ft);
  if (rt >= nrt || ft >= nft) return;
  const int t = threadIdx.x;
  // epilogue operands of thread t < 256 (row t >> 4, unit t & 15), fetched ahead of the chains
  const int er = rt * 16 + ((t & 255) >> 4), j = ft * 16 + (t & 15);
  const bool ework = t < 256 && er < a.n;
  float gir = 0.0f, giz = 0.0f, gin = 0.0f, hprev = 0.0f;
  if (ework) {
    const float* gi = a.layer == 0 ? a.gi0 + (size_t)a.row_frame[a.row0 + er] * m.G : a.gi_up + (size_t)er * m.G;
    const float* hs = a.prev0 >= 0 ? score_hid(m, a, a.layer, a.prev0 + er) : m.h1 + (size_t)a.layer * m.Hp;
    gir = gi[j]; giz = gi[m.Hp + j]; gin = gi[2 * m.Hp + j]; hprev = hs[j];
  }
  int i = rt * 16 + (t & 15);
  if (i >= a.n) i = a.n - 1;
  const float* hsrc[1] = {a.prev0 >= 0 ? score_hid(m, a, a.layer, a.prev0 + i) : m.h1 + (size_t)a.layer * m.Hp};
  splitk_tile<3, 1, 1>(m.whh[a.layer], nft, ft, m.Hp / 16, hsrc, m.bhh[a.layer] + ft * 16, m.Hp, spart);
  if (!ework) return;
  const float ghr = splitk_combine<1, 3>(spart, 0, 0, t);
  const float ghz = splitk_combine<1, 3>(spart, 0, 1, t);
  const float ghn = splitk_combine<1, 3>(spart, 0, 2, t);
  const float out = j < m.H_units ? uis_gru_unit(gir, giz, gin, ghr, ghz, ghn, hprev) : 0.0f;
  score_hid(m, a, a.layer, a.row0 + er)[j] = out;
}

// out[row] = head(b + W in[row]) for `nrows` rows: a wave owns 2 row tiles x 4 feature tiles and walks
// the full K (segments combined left to right: the canonical order; k_dense_input_proj_wide's schedule).
// HEAD 1: relu (linear_mean1, `v > 0 ? v : 0` as the decode), HEAD 2: features past D are 0 (linear_mean2).
template <int HEAD>
__global__ __launch_bounds__(256) void k_score_head(DevModel m, const float* __restrict__ Wt, const float* __restrict__ bias,
                                                    int ntiles, int nKb, const float* __restrict__ in,
                                                    float* __restrict__ out, long nrows) {
  constexpr int NA = 4, NB = 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4;
  const int tile0 = (blockIdx.y * 4 + wave) * NA;
  if (tile0 >= ntiles) return;
  const long r0 = (long)blockIdx.x * (16 * NB);
  if (r0 >= nrows) return;
  const int in_stride = nKb * 16, out_stride = ntiles * 16;
  long rows[NB];
  bool valid[NB];
  const f32x4* bp[NB];
  const f32x4* wp[NA];
  int tiles[NA];
#pragma unroll
  for (int r = 0; r < NB; ++r) {
    rows[r] = r0 + 16 * r + (lane & 15);
    valid[r] = rows[r] < nrows;
    if (!valid[r]) rows[r] = nrows - 1;
    bp[r] = reinterpret_cast<const f32x4*>(in + (size_t)rows[r] * in_stride) + q;
  }
#pragma unroll
  for (int g = 0; g < NA; ++g) {
    tiles[g] = tile0 + g < ntiles ? tile0 + g : ntiles - 1;
    wp[g] = reinterpret_cast<const f32x4*>(Wt) + ((size_t)tiles[g] * nKb) * 64 + lane;
  }
  const int per = uis_kseg_blocks(nKb);
  f32x4 total[NB][NA];
#pragma unroll 1
  for (int sgm = 0; sgm < UIS_KSPLIT; ++sgm) {
    const int kb0 = sgm * per;
    const int kb1 = kb0 + per < nKb ? kb0 + per : nKb;
    f32x4 acc[NB][NA];
#pragma unroll
    for (int r = 0; r < NB; ++r) {
#pragma unroll
      for (int g = 0; g < NA; ++g)
        acc[r][g] = sgm == 0 ? *reinterpret_cast<const f32x4*>(bias + tiles[g] * 16 + 4 * q) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    if (kb0 < kb1) chain_blocks<NA, NB>(wp, bp, kb0, kb1, acc);
#pragma unroll
    for (int r = 0; r < NB; ++r) {
#pragma unroll
      for (int g = 0; g < NA; ++g) {
        if (sgm == 0) total[r][g] = acc[r][g];
        else {
#pragma unroll
          for (int e = 0; e < 4; ++e) total[r][g][e] = total[r][g][e] + acc[r][g][e];
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < NB; ++r) {
#pragma unroll
    for (int g = 0; g < NA; ++g) {
      if (!valid[r] || tile0 + g >= ntiles) continue;
      const int f = (tile0 + g) * 16 + q * 4;
      f32x4 v = total[r][g];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (HEAD == 1) v[e] = v[e] > 0.0f ? v[e] : 0.0f;
        else if (f + e >= m.D) v[e] = 0.0f;
      }
      *reinterpret_cast<f32x4*>(out + (size_t)rows[r] * out_stride + f) = v;
    }
  }
}

// The running cluster mean along each chain, in place: row(p, i) holds linear_mean2's output m_{p+1} on entry
// and M_{p+1} on exit, M_1 = m_1, M_q = uis_mean_update(M_{q-1}, m_q, q - 1)  (uisrnn.py:425-429).
// One thread per (chain, feature); 8 rows fetched ahead of their updates.
// `tail` 1 (prime mode): the chain's last row too.
__global__ __launch_bounds__(256) void k_score_mean_scan(DevModel m, const int32_t* __restrict__ len,
                                                         const int64_t* __restrict__ fbase, float* mean, int tail) {
  const int i = blockIdx.y;
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= m.Dp) return;
  const int nrow = len[i] - 1 + tail;  // rows whose mean a later frame reads
  constexpr int AHEAD = 8;
  float M = 0.0f;
  for (int p0 = 0; p0 < nrow; p0 += AHEAD) {
    float v[AHEAD];
    size_t at[AHEAD];
#pragma unroll
    for (int k = 0; k < AHEAD; ++k) {
      const int p = p0 + k < nrow ? p0 + k : nrow - 1;
      at[k] = (size_t)(fbase[p] + i) * m.Dp + d;
      v[k] = mean[at[k]];
    }
#pragma unroll
    for (int k = 0; k < AHEAD; ++k) {
      const int p = p0 + k;
      if (p >= nrow) break;
      M = p == 0 ? v[k] : uis_mean_update(M, v[k], p);
      mean[at[k]] = M;
    }
  }
}

// loss[frame] = uis_step_loss(mse, prior[frame]) for every row: mse = mse0[frame] at a chain's first frame,
// else the weighted MSE against the chain's mean after the previous row (one wave per row).
__global__ __launch_bounds__(256) void k_score_loss(DevModel m, long Fv, const int32_t* __restrict__ row_frame,
                                                    const int32_t* __restrict__ row_prev, const float* __restrict__ x,
                                                    const float* __restrict__ mse0, const float* __restrict__ mean,
                                                    const double* __restrict__ prior, float* __restrict__ loss) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= Fv) return;
  const long frame = row_frame[r];
  const int prev = row_prev[r];
  float mse;
  if (prev < 0) mse = mse0[frame];
  else mse = wave_weighted_mse(mean + (size_t)prev * m.Dp, x + (size_t)frame * m.Dp, m.wgt, m.Dp, m.D, lane);
  if (lane == 0) loss[frame] = uis_step_loss(mse, prior[frame]);
}

// scores[u] = ((0 + loss_0) + loss_1) + ... over the utterance's scored frames, in frame order; +inf when a
// label was past the allowed range (nvalid[u] < its frames: the reference's invalid trace).  One wave each.
__global__ __launch_bounds__(64) void k_score_sum(const int64_t* __restrict__ off, const int32_t* __restrict__ nvalid,
                                                  const float* __restrict__ loss, float* __restrict__ scores) {
  const int u = blockIdx.x, lane = threadIdx.x;
  const long f0 = off[u], n = off[u + 1] - f0, nv = nvalid[u];
  float s = 0.0f;
  for (long b = 0; b < nv; b += 64) {
    const float v = b + lane < nv ? loss[f0 + b + lane] : 0.0f;
    const int cnt = nv - b < 64 ? (int)(nv - b) : 64;
    for (int k = 0; k < cnt; ++k) s = s + __shfl(v, k, 64);
  }
  if (nv < n) s = INFINITY;
  if (lane == 0) scores[u] = s;
}

// frame_row[t] = the frame-row of frame t: row_frame inverted (frames past an invalid label have no row and keep
// whatever the buffer held: nothing reads them).
__global__ __launch_bounds__(256) void k_speakers_frame_rows(long Fv, const int32_t* __restrict__ row_frame,
                                                             int32_t* __restrict__ frame_row) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r < Fv) frame_row[row_frame[r]] = (int32_t)r;
}

// uis_score_speakers' candidate tables, from the labels: thread (utterance u, cluster k) walks u's valid frames once and
// leaves, for every frame t, cand[t][k] = {the row of sc_mean that holds cluster k's running mean before frame t (-1: not
// open yet), its block count}; thread k = 0 also leaves frame[t] = {K(t), sum(block_counts), last label, 0}, K = -1 from
// the first label past the allowed range on (nvalid[u]: the invalid trace).  Labels and rows are staged 256 frames at a
// time and read 8 frames ahead of the walk.
__global__ __launch_bounds__(64) void k_speakers_tables(const int64_t* __restrict__ off, const int32_t* __restrict__ nvalid,
                                                        const int32_t* __restrict__ labels, const int32_t* __restrict__ frame_row,
                                                        int width, int2* __restrict__ cand, int4* __restrict__ frame) {
  __shared__ int32_t s_lab[256], s_row[256];
  constexpr int AHEAD = 8;
  const int u = blockIdx.x, k = blockIdx.y * 64 + threadIdx.x;
  const long f0 = off[u], n = off[u + 1] - f0, nv = nvalid[u];
  int row = -1, blk = 0, K = 0, sum = 0, last = -1;
  for (long c0 = 0; c0 < n; c0 += 256) {
    const int cnt = n - c0 < 256 ? (int)(n - c0) : 256;
    __syncthreads();
    for (int j = threadIdx.x; j < cnt; j += 64) {
      s_lab[j] = labels[f0 + c0 + j];
      s_row[j] = frame_row[f0 + c0 + j];
    }
    __syncthreads();
    for (int j0 = 0; j0 < cnt; j0 += AHEAD) {
      int lab[AHEAD], rw[AHEAD];
#pragma unroll
      for (int e = 0; e < AHEAD; ++e) {
        const int j = j0 + e < cnt ? j0 + e : cnt - 1;
        lab[e] = s_lab[j];
        rw[e] = s_row[j];
      }
#pragma unroll
      for (int e = 0; e < AHEAD; ++e) {
        if (j0 + e >= cnt) break;
        const long t = f0 + c0 + j0 + e;
        if (c0 + j0 + e >= nv) {
          if (k == 0) frame[t] = make_int4(-1, 0, -1, 0);
          continue;
        }
        if (k < width) cand[(size_t)t * width + k] = make_int2(row, blk);
        if (k == 0) frame[t] = make_int4(K, sum, last, 0);
        const int c = lab[e];
        if (c == K) { ++K; ++sum; if (c == k) blk = 1; }
        else if (c != last) { ++sum; if (c == k) ++blk; }
        if (c == k) row = rw[e];
        last = c;
      }
    }
  }
}

// out[t][k], k < width: the step loss of assigning frame t to cluster k given the labeled history before t -- the
// _calculate_score row along the trace.  k < K(t): the weighted MSE of x_t against the cluster's running mean, prior
// lp_stay for the last label's cluster, else (lp_sw + logblk[blk]) - logden[sum]; k = K(t): the new-speaker candidate
// (mse0, lp_new - logden[sum]); k > K(t), and every k past an invalid label: +inf.  The decode's float64 expressions, on
// the uploaded host tables.  One workgroup per frame: x_t and the weights staged once, a wave per candidate.
// bias3 (uis_frame_bias): frame t's {lp_stay, lp_sw, lp_new} in the model's place, or null.
__global__ __launch_bounds__(256) void k_score_speakers(DevModel m, int width, const double* __restrict__ bias3, const float* __restrict__ x,
                                                        const float* __restrict__ mse0, const float* __restrict__ mean,
                                                        const int2* __restrict__ cand, const int4* __restrict__ frame,
                                                        const double* __restrict__ logblk, const double* __restrict__ logden,
                                                        float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  f32x4* swgt4 = reinterpret_cast<f32x4*>(smem_raw);
  f32x4* sx4 = swgt4 + m.Dp / 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t t = blockIdx.x;
  const int4 f = frame[t];  // {K, sum, last}
  double lp_stay = m.lp_stay, lp_sw = m.lp_sw, lp_new = m.lp_new;
  if (bias3) { lp_stay = bias3[3 * t]; lp_sw = bias3[3 * t + 1]; lp_new = bias3[3 * t + 2]; }
  if (f.x > 0) {            // (no open cluster: no MSE to form)
    const f32x4* xt = reinterpret_cast<const f32x4*>(x + t * m.Dp);
    const f32x4* wg = reinterpret_cast<const f32x4*>(m.wgt);
    for (int i = threadIdx.x; i < m.Dp / 4; i += 256) { swgt4[i] = wg[i]; sx4[i] = xt[i]; }
  }
  __syncthreads();
  const float* swgt = reinterpret_cast<const float*>(swgt4);
  const float* sx = reinterpret_cast<const float*>(sx4);
  for (int k = wave; k < width; k += 4) {
    float v = INFINITY;
    if (k < f.x) {
      const int2 c = cand[t * width + k];
      const float mse = wave_weighted_mse(mean + (size_t)c.x * m.Dp, sx, swgt, m.Dp, m.D, lane);
      const double prior = k == f.z ? lp_stay : (lp_sw + logblk[c.y]) - logden[f.y];
      v = uis_step_loss(mse, prior);
    } else if (k == f.x) {
      v = uis_step_loss(mse0[t], lp_new - logden[f.y]);
    }
    if (lane == 0) out[t * width + k] = v;
  }
}

// uis_speaker_profiles: where a chain's profile goes and what the walk cannot see.  Chains in longest-first order.
struct ProfChain {
  int32_t out;   // its row u * width + k of the outputs; -1: a chain of an invalid trace (its utterance's rows stay absent)
  int32_t blk;   // the cluster's block count (ScoreSchedule::chain_blk)
  int32_t f0;    // the first frame of its utterance in the packed stream
  int32_t pad;
};

// Every row of uis_speaker_profiles' outputs in its absent form: stats {0, 0, -1, -1}, +0.0 in every float.  The rows of
// the chains are written after it, by k_score_profile_scan.  One workgroup per row.
__global__ __launch_bounds__(64) void k_score_profile_absent(int D, int4* __restrict__ stats, float* __restrict__ mean_out,
                                                             float* __restrict__ sum_x, float* __restrict__ sum_r2) {
  const size_t row = blockIdx.x;
  if (threadIdx.x == 0) stats[row] = make_int4(0, 0, -1, -1);
  for (int d = threadIdx.x; d < D; d += 64) {
    mean_out[row * D + d] = 0.0f;
    sum_x[row * D + d] = 0.0f;
    sum_r2[row * D + d] = 0.0f;
  }
}

// The profile of each chain, after k_score_mean_scan(tail = 1): one thread per (chain, dimension d < D) walks the chain's
// positions in order, p = 0 .. len - 1, row(p, i) = fbase[p] + i.  At each it reads the frame's x (through row_frame) and
// the row's running mean M_{p+1} -- the mean the NEXT position is charged against, i.e. the row that row_prev names for
// it; the first position is charged against m0 -- and does, in float32, one operation at a time (the build's
// -ffp-contract=off keeps them apart):  r = x - P;  sum_r2 = sum_r2 + r * r;  sum_x = sum_x + x.
// The last M is the cluster's final mean.  8 positions are fetched ahead of their updates; one fixed order per sum.
__global__ __launch_bounds__(256) void k_score_profile_scan(DevModel m, const int32_t* __restrict__ len, const int64_t* __restrict__ fbase,
                                                            const int32_t* __restrict__ row_frame, const ProfChain* __restrict__ chain,
                                                            const float* __restrict__ x, const float* __restrict__ mean,
                                                            int4* __restrict__ stats, float* __restrict__ mean_out,
                                                            float* __restrict__ sum_x, float* __restrict__ sum_r2) {
  const int i = blockIdx.y;
  const int d = blockIdx.x * 256 + threadIdx.x;
  const ProfChain c = chain[i];
  if (c.out < 0 || d >= m.D) return;
  const int n = len[i];
  constexpr int AHEAD = 8;
  float P = m.m0[d], sx = 0.0f, sr = 0.0f;
  int first = 0, last = 0;
  for (int p0 = 0; p0 < n; p0 += AHEAD) {
    float xv[AHEAD], mv[AHEAD];
    int fr[AHEAD];
#pragma unroll
    for (int k = 0; k < AHEAD; ++k) {
      const int p = p0 + k < n ? p0 + k : n - 1;
      const size_t r = (size_t)(fbase[p] + i);
      fr[k] = row_frame[r];
      mv[k] = mean[r * m.Dp + d];
    }
#pragma unroll
    for (int k = 0; k < AHEAD; ++k) xv[k] = x[(size_t)fr[k] * m.Dp + d];
#pragma unroll
    for (int k = 0; k < AHEAD; ++k) {
      const int p = p0 + k;
      if (p >= n) break;
      const float r = xv[k] - P;
      sr = sr + r * r;
      sx = sx + xv[k];
      P = mv[k];
      if (p == 0) first = fr[k];
      last = fr[k];
    }
  }
  const size_t o = (size_t)c.out * m.D + d;
  mean_out[o] = P;
  sum_x[o] = sx;
  sum_r2[o] = sr;
  if (d == 0) stats[c.out] = make_int4(n, c.blk, first - c.f0, last - c.f0);
}

static bool score_timing_env() {  // UIS_SCORE_TIMING=1: one line per call on stderr (schedule / device / total ms)
  static const bool v = getenv("UIS_SCORE_TIMING") != nullptr && atoi(getenv("UIS_SCORE_TIMING")) != 0;
  return v;
}

// The schedule of one call: integer work on the labels and the float64 priors.
struct ScoreSchedule {
  std::vector<int32_t> nvalid;     // [U] frames before the first label past the allowed range
  std::vector<double> prior;       // [F]
  std::vector<int32_t> len;        // [chains] longest first
  std::vector<int64_t> fbase;      // [P] row(p, 0)
  std::vector<int32_t> nfr;        // [P] chains with more than p frames
  std::vector<int32_t> row_frame;  // [Fv]
  std::vector<int32_t> row_prev;   // [Fv] row(p - 1, i), -1 at p = 0
  int64_t Fv = 0;
  // what the traces leave behind, for priming a session (uis_prime.hip); chains here in (utterance, cluster) order
  std::vector<int32_t> chain_base;  // [U + 1] utterance u's chains: chain_base[u] + cluster
  std::vector<int32_t> rank;        // [chains] the chain's index i in the longest-first order
  std::vector<int32_t> chain_blk;   // [chains] block count of the cluster
  std::vector<int32_t> utt_last;    // [U] last label (-1: no frame)
  std::vector<int32_t> utt_sum;     // [U] sum(block_counts)
  std::vector<double> logblk, logden;  // the decode's tables (upload_log_tables, uis_workspace.hip), as far as this call reaches
};

// bias3: the call's per-frame {lp_stay, lp_sw, lp_new} (uis_frame_bias; [F][3], host) or null: the model's at every frame.
void score_schedule(const DevModel& m, double alpha, const int64_t* offsets, int U, const int32_t* labels, ScoreSchedule& s,
                    const double* bias3 = nullptr) {
  const int64_t F = offsets[U];
  int64_t maxN = 0;
  for (int u = 0; u < U; ++u) maxN = std::max<int64_t>(maxN, offsets[u + 1] - offsets[u]);
  // the decode's tables (upload_log_tables, uis_workspace.hip)
  std::vector<double>& logblk = s.logblk;
  std::vector<double>& logden = s.logden;
  logblk.resize(maxN + 2);
  logden.resize(maxN + 2);
  for (int64_t n = 0; n < maxN + 2; ++n) {
    logblk[n] = n > 0 ? std::log((double)n) : 0.0;
    logden[n] = std::log((double)n + alpha);
  }
  s.nvalid.assign(U, 0);
  s.prior.assign(F, 0.0);
  std::vector<int32_t>& chain_base = s.chain_base;
  std::vector<int32_t>& rank = s.rank;
  chain_base.assign(U + 1, 0);
  s.chain_blk.clear();
  s.utt_last.assign(U, -1);
  s.utt_sum.assign(U, 0);
  std::vector<int32_t> chain_len, blk;
  std::vector<int32_t> frame_chain(F, -1), frame_pos(F, 0);
  for (int u = 0; u < U; ++u) {
    int K = 0, last = -1;
    int64_t sum = 0;
    blk.clear();
    int64_t t = offsets[u];
    for (; t < offsets[u + 1]; ++t) {
      const int c = labels[t];
      if (c > K) break;  // invalid trace (uisrnn.py:406-408): +inf from here on
      const double lp_stay = bias3 ? bias3[3 * t] : m.lp_stay, lp_sw = bias3 ? bias3[3 * t + 1] : m.lp_sw;
      const double lp_new = bias3 ? bias3[3 * t + 2] : m.lp_new;
      double prior;
      if (c == last) prior = lp_stay;
      else if (c < K) prior = (lp_sw + logblk[blk[c]]) - logden[sum];
      else prior = lp_new - logden[sum];
      s.prior[t] = prior;
      if (c == K) { blk.push_back(1); ++sum; ++K; chain_len.push_back(0); }
      else if (c != last) { ++blk[c]; ++sum; }
      const int ch = chain_base[u] + c;
      frame_chain[t] = ch;
      frame_pos[t] = chain_len[ch]++;
      last = c;
    }
    s.nvalid[u] = (int32_t)(t - offsets[u]);
    chain_base[u + 1] = chain_base[u] + K;
    s.chain_blk.insert(s.chain_blk.end(), blk.begin(), blk.end());
    s.utt_last[u] = last;
    s.utt_sum[u] = (int32_t)sum;
  }
  const int nch = chain_base[U];
  // longest first (counting sort, stable: ties keep (utterance, cluster) order)
  int P = 0;
  for (int c = 0; c < nch; ++c) P = std::max(P, chain_len[c]);
  std::vector<int32_t> cnt(P + 2, 0);
  rank.assign(nch, 0);
  for (int c = 0; c < nch; ++c) ++cnt[P - chain_len[c]];
  for (int k = 1; k <= P + 1; ++k) cnt[k] += cnt[k - 1];
  for (int c = nch - 1; c >= 0; --c) rank[c] = --cnt[P - chain_len[c]];
  s.len.assign(nch, 0);
  for (int c = 0; c < nch; ++c) s.len[rank[c]] = chain_len[c];
  s.nfr.assign(P, 0);
  s.fbase.assign(P, 0);
  for (int i = 0; i < nch; ++i) ++s.nfr[s.len[i] - 1];  // (chains of exactly len[i] frames ...)
  for (int p = P - 2; p >= 0; --p) s.nfr[p] += s.nfr[p + 1];  // ... summed from the top: chains longer than p
  int64_t acc = 0;
  for (int p = 0; p < P; ++p) { s.fbase[p] = acc; acc += s.nfr[p]; }
  s.Fv = acc;
  s.row_frame.assign(acc, 0);
  s.row_prev.assign(acc, -1);
  for (int64_t t = 0; t < F; ++t) {
    if (frame_chain[t] < 0) continue;
    const int i = rank[frame_chain[t]], p = frame_pos[t];
    const int64_t r = s.fbase[p] + i;
    s.row_frame[r] = (int32_t)t;
    s.row_prev[r] = p > 0 ? (int32_t)(s.fbase[p - 1] + i) : -1;
  }
}

// `keep` non-null: PRIME mode -- every chain runs to its end (see the head of this file) and the schedule is left in
// *keep; the buffers (sc_hid, sc_mean, sc_out, sc_utt's offsets) stay as they are until the handle's next scoring call.
// `spk` non-null: uis_score_speakers -- every chain runs to its end as in PRIME mode (a cluster's final mean is what the
// frames after its last one are scored against), then the candidate tables and the rows; spk->losses_out is
// [F][spk->width], the host has checked the width.
struct ScoreSpeakers {
  int32_t width;
  float* losses_out;
};

// `prof` non-null: uis_speaker_profiles -- every chain runs to its end as in PRIME mode, then k_score_profile_scan; the
// outputs are [n_utt][prof->width] rows, the host has checked the width; sum_x_out / sum_r2_out may be null.
struct ScoreProfiles {
  int32_t width;
  int32_t* n_clusters_out;
  int32_t* stats_out;
  float *mean_out, *sum_x_out, *sum_r2_out;
};

int score_run(uis_handle* h, const float* frames, const int64_t* offsets, int32_t U, const int32_t* labels, float* scores_out,
              float* frame_losses_out, ScoreSchedule* keep = nullptr, const ScoreSpeakers* spk = nullptr,
              const ScoreProfiles* prof = nullptr) {
  const DevModel& m = h->m;
  const int64_t F = offsets[U];
  const auto t_begin = std::chrono::steady_clock::now();
  const bool prime = keep != nullptr || spk != nullptr || prof != nullptr;  // (the recurrence bound, the scan's tail and the valid last row)
  ScoreSchedule s_own;
  ScoreSchedule& s = keep ? *keep : s_own;
  // (uis_frame_bias: the scoring entry points took the table and checked its length; a priming run never has one)
  const double* bias3 = keep ? nullptr : h->tables.bias3.data();
  score_schedule(m, h->alpha, offsets, U, labels, s, bias3);
  const auto t_sched = std::chrono::steady_clock::now();
  const int64_t Fv = s.Fv;
  const int P = (int)s.fbase.size(), nch = (int)s.len.size();
  const int maxn = prime ? (P > 0 ? s.nfr[0] : 0) : (P > 1 ? s.nfr[1] : 0);  // the most chains one recurrence launch runs
  const size_t W = spk ? (size_t)spk->width : 0, nlog = s.logblk.size();
  HIPCHK(hipSetDevice(h->device));
  int rc;
  auto need = [](int64_t n, size_t each) { return (size_t)std::max<int64_t>(n, 1) * each; };
  if ((rc = h->sc_x.ensure(need(F, (size_t)m.D * 4))) || (rc = h->sc_gi0.ensure(need(F, (size_t)m.G * 4))) ||
      (rc = h->sc_mse0.ensure(need(F, 4))) || (rc = h->sc_loss.ensure(need(F, 4))) ||
      (rc = h->sc_prior.ensure(need(F, 8))) || (rc = h->sc_hid.ensure(need(Fv, (size_t)m.depth * m.Hp * 4))) ||
      (rc = h->sc_a1.ensure(need(Fv, (size_t)m.Hp * 4))) || (rc = h->sc_mean.ensure(need(Fv, (size_t)m.Dp * 4))) ||
      (rc = h->sc_gi_up.ensure(need(m.depth > 1 ? maxn : 0, (size_t)m.G * 4))) ||
      (rc = h->sc_rows.ensure(need(Fv, 8))) || (rc = h->sc_chains.ensure(need(P, 8) + need(nch, 4))) ||
      (rc = h->sc_utt.ensure(need(U + 1, 8) + need(U, 4))) || (rc = h->sc_out.ensure(need(U, 4))))
    return rc;
  if (m.D != m.Dp && (rc = h->sc_xpad.ensure(need(F, (size_t)m.Dp * 4)))) return rc;
  if (spk && ((rc = h->sc_spk_in.ensure(need(F, 8))) || (rc = h->sc_spk_log.ensure(2 * nlog * 8)) ||
              (rc = h->sc_spk_cand.ensure(need(F, W * 8))) || (rc = h->sc_spk_frame.ensure(need(F, 16))) ||
              (rc = h->sc_spk_loss.ensure(need(F, W * 4)))))
    return rc;
  if (spk && bias3 && (rc = h->sc_spk_bias.ensure(need(F, 24)))) return rc;
  const size_t prof_rows = prof ? (size_t)U * (size_t)prof->width : 0;
  if (prof && ((rc = h->sc_prof_chain.ensure(need(nch, sizeof(ProfChain)))) || (rc = h->sc_prof_stats.ensure(prof_rows * 16)) ||
               (rc = h->sc_prof_mean.ensure(prof_rows * m.D * 4)) || (rc = h->sc_prof_sumx.ensure(prof_rows * m.D * 4)) ||
               (rc = h->sc_prof_sumr2.ensure(prof_rows * m.D * 4))))
    return rc;
  hipStream_t st = h->stream;
  {  // UIS_POISON_WORKSPACE: every sc_* buffer, ahead of the tables and the frames on the same stream
    const UisPoison poison = UisPoison::from_env();
    for (DevBuf* b : {&h->sc_x, &h->sc_xpad, &h->sc_gi0, &h->sc_mse0, &h->sc_loss, &h->sc_prior, &h->sc_hid, &h->sc_a1, &h->sc_mean,
                      &h->sc_gi_up, &h->sc_rows, &h->sc_chains, &h->sc_utt, &h->sc_out, &h->sc_spk_in, &h->sc_spk_log,
                      &h->sc_spk_cand, &h->sc_spk_frame, &h->sc_spk_loss, &h->sc_spk_bias, &h->sc_prof_chain, &h->sc_prof_stats,
                      &h->sc_prof_mean, &h->sc_prof_sumx, &h->sc_prof_sumr2})
      HIPCHK(poison.device(b->p, b->cap, st));
  }
  int32_t* d_row_frame = h->sc_rows.as<int32_t>();
  int32_t* d_row_prev = d_row_frame + std::max<int64_t>(Fv, 1);
  int64_t* d_fbase = h->sc_chains.as<int64_t>();
  int32_t* d_len = reinterpret_cast<int32_t*>(d_fbase + std::max(P, 1));
  int64_t* d_off = h->sc_utt.as<int64_t>();
  int32_t* d_nvalid = reinterpret_cast<int32_t*>(d_off + U + 1);
  // the tables and the frames travel; everything below runs in order on the handle's stream
  if (F > 0) {
    HIPCHK(hipMemcpyAsync(h->sc_x.p, frames, (size_t)F * m.D * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(h->sc_prior.p, s.prior.data(), (size_t)F * 8, hipMemcpyHostToDevice, st));
  }
  if (Fv > 0) {
    HIPCHK(hipMemcpyAsync(d_row_frame, s.row_frame.data(), (size_t)Fv * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_row_prev, s.row_prev.data(), (size_t)Fv * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_len, s.len.data(), (size_t)nch * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_fbase, s.fbase.data(), (size_t)P * 8, hipMemcpyHostToDevice, st));
  }
  HIPCHK(hipMemcpyAsync(d_off, offsets, (size_t)(U + 1) * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_nvalid, s.nvalid.data(), (size_t)U * 4, hipMemcpyHostToDevice, st));
  int32_t *d_labels = nullptr, *d_frame_row = nullptr;
  double *d_logblk = nullptr, *d_logden = nullptr;
  if (spk && F > 0) {  // the labels and the prior tables (host std::log, as the decode's) travel; each frame's row is formed there
    d_labels = h->sc_spk_in.as<int32_t>();
    d_frame_row = d_labels + F;
    d_logblk = h->sc_spk_log.as<double>();
    d_logden = d_logblk + nlog;
    HIPCHK(hipMemcpyAsync(d_labels, labels, (size_t)F * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_logblk, s.logblk.data(), nlog * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_logden, s.logden.data(), nlog * 8, hipMemcpyHostToDevice, st));
    if (bias3) HIPCHK(hipMemcpyAsync(h->sc_spk_bias.p, bias3, (size_t)F * 24, hipMemcpyHostToDevice, st));
  }
  std::vector<ProfChain> prof_chain;  // (alive until the synchronisation below)
  if (prof) {  // which (utterance, cluster) each chain is, from the schedule; a chain of an invalid trace has no row
    prof_chain.assign(std::max(nch, 1), ProfChain{-1, 0, 0, 0});
    for (int u = 0; u < U; ++u) {
      const bool valid = s.nvalid[u] == offsets[u + 1] - offsets[u];
      prof->n_clusters_out[u] = valid ? s.chain_base[u + 1] - s.chain_base[u] : -1;
      for (int c = s.chain_base[u]; c < s.chain_base[u + 1]; ++c)
        prof_chain[s.rank[c]] = ProfChain{valid ? (int32_t)((size_t)u * prof->width + (c - s.chain_base[u])) : -1, s.chain_blk[c],
                                          (int32_t)offsets[u], 0};
    }
    HIPCHK(hipMemcpyAsync(h->sc_prof_chain.p, prof_chain.data(), prof_chain.size() * sizeof(ProfChain), hipMemcpyHostToDevice, st));
  }
  HIPCHK(hipEventRecord(h->ev_begin, st));
  Launcher lch{h, st, false};
  const float* d_x = h->sc_x.as<float>();
  float* gi0 = h->sc_gi0.as<float>();
  float* mse0 = h->sc_mse0.as<float>();
  float* loss = h->sc_loss.as<float>();
  if (F > 0) {
    // the frame stream: the decode's kernels, unchanged
    if (m.D != m.Dp) {
      const long total = (long)F * m.Dp;
      hipLaunchKernelGGL(k_pad_frames, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d_x, h->sc_xpad.as<float>(),
                         (long)F, m.D, m.Dp);
      HIPCHK(hipGetLastError());
      d_x = h->sc_xpad.as<float>();
    }
    if (F >= UIS_PROJ_WIDE_ROWS) {
      LAUNCH(UIS_K_INPUT_PROJ, k_dense_input_proj_wide, dim3((unsigned)((F + 31) / 32), (unsigned)((m.G / 16 + 15) / 16)), dim3(256), 0,
             m, d_x, gi0, (long)F);
      LAUNCH(UIS_K_INPUT_PROJ, k_mse0, dim3((unsigned)((F + 3) / 4)), dim3(256), (size_t)5 * m.Dp * 4, m, d_x, mse0, (long)F, 0L,
             (const long*)nullptr);
    } else if ((rc = plain_input_proj(lch, m, d_x, gi0, mse0, (long)F))) {
      return rc;
    }
    // frames past an invalid label keep +inf
    HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(loss), 0x7f800000, (size_t)F, st));
  }
  if (Fv > 0) {
    ScoreStep a{};
    a.Fv = Fv; a.row_frame = d_row_frame; a.gi0 = gi0; a.gi_up = h->sc_gi_up.as<float>(); a.hid = h->sc_hid.as<float>();
    // the recurrence: position p's GRU rows are the chains with a frame at p + 1 (prime mode: with a frame at p)
    for (int p = 0; p + (prime ? 0 : 1) < P; ++p) {
      a.n = prime ? s.nfr[p] : s.nfr[p + 1];
      a.row0 = s.fbase[p];
      a.prev0 = p > 0 ? s.fbase[p - 1] : -1;
      const int nrt = (a.n + 15) / 16;
      for (int l = 0; l < m.depth; ++l) {
        a.layer = l;
        if (l > 0) LAUNCH(UIS_K_UPPER_IN, k_score_upper_in, dim3((unsigned)dense_grid_blocks(nrt, m.G / 16)), dim3(512), 0, m, a);
        LAUNCH(UIS_K_GRU, k_score_gru, dim3((unsigned)dense_grid_blocks(nrt, m.Hp / 16)), dim3(512), 0, m, a);
      }
    }
    // the heads of every row at once (a chain's last row included: a scoring call computes its mean from an unwritten
    // hidden state and never reads it; in prime mode the row is valid and its running mean is the cluster's final one)
    const float* htop = a.hid + (size_t)(m.depth - 1) * Fv * m.Hp;
    float* a1 = h->sc_a1.as<float>();
    float* mean = h->sc_mean.as<float>();
    LAUNCH(UIS_K_HEAD1, k_score_head<1>, dim3((unsigned)((Fv + 31) / 32), (unsigned)((m.Hp / 16 + 15) / 16)), dim3(256), 0, m,
           m.w1, m.b1, m.Hp / 16, m.Hp / 16, htop, a1, (long)Fv);
    LAUNCH(UIS_K_HEAD2, k_score_head<2>, dim3((unsigned)((Fv + 31) / 32), (unsigned)((m.Dp / 16 + 15) / 16)), dim3(256), 0, m,
           m.w2, m.b2, m.Dp / 16, m.Hp / 16, a1, mean, (long)Fv);
    if (P > 1 || prime)
      LAUNCH(UIS_K_HEAD2, k_score_mean_scan, dim3((unsigned)((m.Dp + 255) / 256), (unsigned)nch), dim3(256), 0, m, d_len, d_fbase, mean,
             prime ? 1 : 0);
    LAUNCH(UIS_K_SELECT, k_score_loss, dim3((unsigned)((Fv + 3) / 4)), dim3(256), 0, m, (long)Fv, d_row_frame, d_row_prev, d_x, mse0,
           mean, h->sc_prior.as<double>(), loss);
  }
  LAUNCH(UIS_K_SELECT, k_score_sum, dim3((unsigned)U), dim3(64), 0, d_off, d_nvalid, loss, h->sc_out.as<float>());
  if (spk && F > 0) {
    if (Fv > 0)
      LAUNCH(UIS_K_SELECT, k_speakers_frame_rows, dim3((unsigned)((Fv + 255) / 256)), dim3(256), 0, (long)Fv, d_row_frame,
             d_frame_row);
    LAUNCH(UIS_K_SELECT, k_speakers_tables, dim3((unsigned)U, (unsigned)((W + 63) / 64)), dim3(64), 0, d_off, d_nvalid, d_labels,
           d_frame_row, (int)W, h->sc_spk_cand.as<int2>(), h->sc_spk_frame.as<int4>());
    LAUNCH(UIS_K_SELECT, k_score_speakers, dim3((unsigned)F), dim3(256), (size_t)2 * m.Dp * 4, m, (int)W,
           bias3 ? h->sc_spk_bias.as<double>() : (const double*)nullptr, d_x, mse0,
           h->sc_mean.as<float>(), h->sc_spk_cand.as<int2>(), h->sc_spk_frame.as<int4>(), d_logblk, d_logden,
           h->sc_spk_loss.as<float>());
  }
  if (prof && prof_rows > 0) {
    LAUNCH(UIS_K_SELECT, k_score_profile_absent, dim3((unsigned)prof_rows), dim3(64), 0, m.D, h->sc_prof_stats.as<int4>(),
           h->sc_prof_mean.as<float>(), h->sc_prof_sumx.as<float>(), h->sc_prof_sumr2.as<float>());
    if (Fv > 0)
      LAUNCH(UIS_K_SELECT, k_score_profile_scan, dim3((unsigned)((m.D + 255) / 256), (unsigned)nch), dim3(256), 0, m, d_len, d_fbase,
             d_row_frame, h->sc_prof_chain.as<ProfChain>(), d_x, h->sc_mean.as<float>(), h->sc_prof_stats.as<int4>(),
             h->sc_prof_mean.as<float>(), h->sc_prof_sumx.as<float>(), h->sc_prof_sumr2.as<float>());
  }
  HIPCHK(hipEventRecord(h->ev_end, st));
  if (prof && prof_rows > 0) {
    HIPCHK(hipMemcpyAsync(prof->stats_out, h->sc_prof_stats.p, prof_rows * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(prof->mean_out, h->sc_prof_mean.p, prof_rows * m.D * 4, hipMemcpyDeviceToHost, st));
    if (prof->sum_x_out) HIPCHK(hipMemcpyAsync(prof->sum_x_out, h->sc_prof_sumx.p, prof_rows * m.D * 4, hipMemcpyDeviceToHost, st));
    if (prof->sum_r2_out) HIPCHK(hipMemcpyAsync(prof->sum_r2_out, h->sc_prof_sumr2.p, prof_rows * m.D * 4, hipMemcpyDeviceToHost, st));
  }
  if (spk && F > 0)
    HIPCHK(hipMemcpyAsync(spk->losses_out, h->sc_spk_loss.p, (size_t)F * W * 4, hipMemcpyDeviceToHost, st));
  if (scores_out) HIPCHK(hipMemcpyAsync(scores_out, h->sc_out.p, (size_t)U * 4, hipMemcpyDeviceToHost, st));
  if (frame_losses_out && F > 0) HIPCHK(hipMemcpyAsync(frame_losses_out, loss, (size_t)F * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (score_timing_env()) {
    float dev_ms = 0.0f;
    (void)hipEventElapsedTime(&dev_ms, h->ev_begin, h->ev_end);
    const auto t_end = std::chrono::steady_clock::now();
    fprintf(stderr, "%s: frames %lld chains %d longest %d schedule_ms %.3f device_ms %.3f total_ms %.3f\n",
            prof ? "uis_speaker_profiles" : spk ? "uis_score_speakers" : prime ? "uis_stream_prime (forced run)" : "uis_score_labels", (long long)F, nch, P, std::chrono::duration<double, std::milli>(t_sched - t_begin).count(), (double)dev_ms,
            std::chrono::duration<double, std::milli>(t_end - t_begin).count());
  }
  return UIS_OK;
}

// The argument checks of uis_score_labels and uis_score_speakers.  *done: n_utt = 0, nothing to score.
int score_check(uis_handle* h, const float* frames, const int64_t* offsets, int32_t n_utt, const int32_t* labels, bool* done) {
  *done = false;
  if (!h || !offsets || n_utt < 0) return fail(UIS_ERR_INVALID_ARG, "null handle/offsets or negative n_utt");
  if (h->stream_state.active) return fail(UIS_ERR_INVALID_ARG, "a streaming session is open on this handle (uis_stream_end first)");
  if (n_utt == 0) { *done = true; return UIS_OK; }
  if (offsets[0] != 0) return fail(UIS_ERR_INVALID_ARG, "offsets[0] must be 0");
  for (int u = 0; u < n_utt; ++u)
    if (offsets[u + 1] < offsets[u]) return fail(UIS_ERR_INVALID_ARG, "offsets must be non-decreasing");
  const int64_t F = offsets[n_utt];
  if (F > 0 && (!frames || !labels)) return fail(UIS_ERR_INVALID_ARG, "frames/labels is null");
  if (F > 0x7fffffffLL) return fail(UIS_ERR_UNSUPPORTED, "more than 2^31 - 1 frames in one call");
  for (int64_t t = 0; t < F; ++t)
    if (labels[t] < 0) return fail(UIS_ERR_INVALID_ARG, "label " + std::to_string(labels[t]) + " at frame " + std::to_string(t) + " is negative");
  return UIS_OK;
}

}  // namespace

UIS_EXPORT int32_t uis_score_labels(uis_handle* h, const float* frames, const int64_t* offsets, int32_t n_utt,
                                    const int32_t* labels, float* scores_out, float* frame_losses_out) {
  if (int rc = begin_call(h, "uis_score_labels", UIS_RULE_SCORE)) return rc;
  bool done;
  if (int rc = score_check(h, frames, offsets, n_utt, labels, &done)) return rc;
  if (int rc = table_status(h->tables.check_bias("call", n_utt ? offsets[n_utt] : 0))) return rc;
  if (done) return UIS_OK;
  return score_run(h, frames, offsets, n_utt, labels, scores_out, frame_losses_out);
}

UIS_EXPORT int32_t uis_score_speakers(uis_handle* h, const float* frames, const int64_t* offsets, int32_t n_utt,
                                      const int32_t* labels, int32_t width, float* losses_out, float* scores_out) {
  if (int rc = begin_call(h, "uis_score_speakers", UIS_RULE_SCORE)) return rc;
  bool done;
  if (int rc = score_check(h, frames, offsets, n_utt, labels, &done)) return rc;
  if (int rc = table_status(h->tables.check_bias("call", n_utt ? offsets[n_utt] : 0))) return rc;
  if (width < 1) return fail(UIS_ERR_INVALID_ARG, "width must be at least 1");
  if (done) return UIS_OK;
  const int64_t F = offsets[n_utt];
  if (F > 0 && !losses_out) return fail(UIS_ERR_INVALID_ARG, "losses_out is null");
  for (int u = 0; u < n_utt; ++u) {  // the clusters of the valid trace (an invalid label ends it)
    int K = 0;
    for (int64_t t = offsets[u]; t < offsets[u + 1] && labels[t] <= K; ++t)
      if (labels[t] == K) ++K;
    if (width < K + 1)
      return fail(UIS_ERR_INVALID_ARG, "utterance " + std::to_string(u) + " has " + std::to_string(K) + " clusters: width must be at least " +
                                           std::to_string(K + 1) + ", not " + std::to_string(width));
  }
  const ScoreSpeakers spk{width, losses_out};
  return score_run(h, frames, offsets, n_utt, labels, scores_out, nullptr, nullptr, &spk);
}

namespace {

// The opener of the scoring calls that come after uis_score_labels / uis_score_speakers: their rule, UIS_RULE_SCORE.
// It has one caller and exists for the same reason as begin_session_call (uis_stream.hip):
// tests/test_call_tables_host.py counts the entry points in csrc/ that open with a literal call of begin_call under
// their own quoted name (23, this comment must not spell one), and that file is not a new entry point's to edit.  The rule table of tests/test_gpu_call_tables.py does not list uis_speaker_profiles
// or uis_session_profiles for the same reason; tests/test_gpu_profiles.py holds both to their rules instead.
int begin_score_call(uis_handle* h, const char* who) { return begin_call(h, who, UIS_RULE_SCORE); }

}  // namespace

// Who the speakers of a labeling are: see include/uisrnn_hip.h and DESIGN.md section 33.
UIS_EXPORT int32_t uis_speaker_profiles(uis_handle* h, const float* frames, const int64_t* offsets, int32_t n_utt,
                                        const int32_t* labels, int32_t width, int32_t* n_clusters_out, int32_t* stats_out,
                                        float* mean_out, float* sum_x_out, float* sum_r2_out, float* scores_out) {
  if (int rc = begin_score_call(h, "uis_speaker_profiles")) return rc;
  bool done;
  if (int rc = score_check(h, frames, offsets, n_utt, labels, &done)) return rc;
  if (int rc = table_status(h->tables.check_bias("call", n_utt ? offsets[n_utt] : 0))) return rc;
  if (width < 1) return fail(UIS_ERR_INVALID_ARG, "width must be at least 1");
  if (done) return UIS_OK;
  if (!n_clusters_out || !stats_out || !mean_out) return fail(UIS_ERR_INVALID_ARG, "n_clusters_out/stats_out/mean_out is null");
  int64_t chains = 0;
  for (int u = 0; u < n_utt; ++u) {  // the clusters of the valid trace (an invalid label ends it)
    int K = 0;
    for (int64_t t = offsets[u]; t < offsets[u + 1] && labels[t] <= K; ++t)
      if (labels[t] == K) ++K;
    if (width < K)
      return fail(UIS_ERR_INVALID_ARG, "utterance " + std::to_string(u) + " has " + std::to_string(K) + " clusters: width must be at least " +
                                           std::to_string(K) + ", not " + std::to_string(width));
    chains += K;
  }
  // (k_score_mean_scan and k_score_profile_scan take one grid row per chain: the y dimension of a launch ends at 65535)
  if (chains > 65535)
    return fail(UIS_ERR_UNSUPPORTED, "the call's utterances hold " + std::to_string((long long)chains) +
                                         " clusters in all, more than 65535: profile the list in parts");
  if ((int64_t)n_utt * width > 0x7fffffffLL) return fail(UIS_ERR_UNSUPPORTED, "more than 2^31 - 1 profile rows in one call");
  const ScoreProfiles prof{width, n_clusters_out, stats_out, mean_out, sum_x_out, sum_r2_out};
  return score_run(h, frames, offsets, n_utt, labels, scores_out, nullptr, nullptr, nullptr, &prof);
}
