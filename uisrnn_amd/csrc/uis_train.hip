// uis_train.hip -- one training iteration of UIS-RNN on gfx950 (include/uisrnn_hip.h: uis_train_*).
//
// The arithmetic of UISRNN.fit_concatenated's loop (uisrnn/uisrnn.py:254-296) and of
// uisrnn/loss_func.py, restated for the device:
//   gather     X0[t, b] = 0 at t = 0, row t-1 of sub-sequence b while t < len_b, else 0
//   GRU        per layer: Gi = X W_ihᵀ + b_ih for all T·B rows (k_gemm), then one launch per step
//              (k_gru_fwd_step) for  r, z = σ(Gi + W_hh h + b_hh),  n = tanh(Gi_n + r ⊙ (W_hn h + b_hn)),
//              h' = n + z ⊙ (h - n); a column past its length keeps its state and outputs 0
//   head       mean = W2 relu(W1 y + b1) + b2 for all rows, cumsum over time / (t+1)
//   losses     loss1 = Σ w_d diff² / nz, loss2 the inverse-gamma prior, loss3 = reg · Σ ‖p‖_F
//   backward   reverse cumsum, head backward (GEMMs), one launch per reverse step per layer
//              (k_gru_bwd_step) carrying dh, weight gradients as GEMMs over all steps
//   update     clip_grad_norm_ over CoreRNN's parameters, Adam (torch's order), sigma2 >= 1e-6
//
// Every reduction has a fixed order (no float atomics): two runs with the same batches give
// bit-identical weights.  Everything runs on the trainer's own stream.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "uis_poison.h"
#include "uisrnn_hip.h"

#define UIS_EXPORT extern "C" __attribute__((visibility("default")))

int uis_internal_fail(int code, const std::string& msg);  // uis_decoder.hip

namespace {

int tfail(int code, const std::string& msg) { return uis_internal_fail(code, msg); }

#define TCHK(expr)                                                                     \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess)                                                              \
      return tfail(e_ == hipErrorOutOfMemory ? UIS_ERR_OOM : UIS_ERR_HIP,              \
                   std::string(#expr) + ": " + hipGetErrorString(e_));                 \
  } while (0)

constexpr int kTile = 64;    // k_gemm: 64 x 64 outputs per workgroup, 4 x 4 per thread
constexpr int kTileK = 16;
constexpr int kChunk = 1024; // step kernels: LDS chunk of the reduction vector

// ---------------------------------------------------------------------------------------------
// C[m, n] = Σ_k A(m, k) B(k, n) (+ bias[n]),  A(m, k) = A[m·sam + k·sak],  B(k, n) = B[k·sbk + n·sbn].
// One fixed summation order per output (k ascending, fmaf), whatever the launch.
__global__ __launch_bounds__(256) void k_gemm(int64_t M, int64_t N, int64_t K,
                                              const float* __restrict__ A, int64_t sam, int64_t sak,
                                              const float* __restrict__ B, int64_t sbk, int64_t sbn,
                                              float* __restrict__ C, int64_t ldc,
                                              const float* __restrict__ bias) {
  __shared__ float As[kTileK][kTile + 1];
  __shared__ float Bs[kTileK][kTile + 1];
  const int tid = threadIdx.x;
  const int tx = tid % 16, ty = tid / 16;
  const int64_t m0 = (int64_t)blockIdx.x * kTile, n0 = (int64_t)blockIdx.y * kTile;
  float acc[4][4];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int64_t k0 = 0; k0 < K; k0 += kTileK) {
    for (int e = tid; e < kTile * kTileK; e += 256) {
      // A: consecutive threads walk m when A is m-contiguous, k otherwise
      int mm, kk;
      if (sam == 1) { mm = e % kTile; kk = e / kTile; } else { kk = e % kTileK; mm = e / kTileK; }
      const int64_t m = m0 + mm, k = k0 + kk;
      As[kk][mm] = (m < M && k < K) ? A[m * sam + k * sak] : 0.f;
      int nn, kb;
      if (sbn == 1) { nn = e % kTile; kb = e / kTile; } else { kb = e % kTileK; nn = e / kTileK; }
      const int64_t n = n0 + nn, kB = k0 + kb;
      Bs[kb][nn] = (n < N && kB < K) ? B[kB * sbk + n * sbn] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kTileK; ++kk) {
      float a[4], b[4];
      for (int i = 0; i < 4; ++i) a[i] = As[kk][ty + 16 * i];
      for (int j = 0; j < 4; ++j) b[j] = Bs[kk][tx + 16 * j];
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }
  for (int i = 0; i < 4; ++i) {
    const int64_t m = m0 + ty + 16 * i;
    if (m >= M) continue;
    for (int j = 0; j < 4; ++j) {
      const int64_t n = n0 + tx + 16 * j;
      if (n < N) C[m * ldc + n] = bias ? acc[i][j] + bias[n] : acc[i][j];
    }
  }
}

// Column sums of a [rows, cols] matrix: 64 columns per workgroup, four row slices summed in order.
__global__ __launch_bounds__(256) void k_colsum(int64_t rows, int64_t cols, const float* __restrict__ X,
                                                float* __restrict__ out) {
  __shared__ float part[4][64];
  const int c = threadIdx.x % 64, s = threadIdx.x / 64;
  const int64_t col = (int64_t)blockIdx.x * 64 + c;
  float acc = 0.f;
  if (col < cols)
    for (int64_t r = s; r < rows; r += 4) acc += X[r * cols + col];
  part[s][c] = acc;
  __syncthreads();
  if (s == 0 && col < cols) out[col] = ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
}

// Fixed-order tree sum of one value per thread of a 256-thread block (result valid in thread 0).
__device__ float block_sum(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// Frobenius norms of the segments of a flat vector, in two passes with one fixed order.
// Pass 1: workgroup (chunk c, segment s) sums the squares of kNormChunk elements of segment s into
// partial[s * n_chunks + c] (0 past the segment's end).  Pass 2: one workgroup per segment adds its
// partials in chunk order and takes the square root.
constexpr int kNormChunk = 4096;

__global__ __launch_bounds__(256) void k_seg_sq_partial(const float* __restrict__ v, const int64_t* __restrict__ seg_off,
                                                        const int64_t* __restrict__ seg_len, int n_chunks,
                                                        float* __restrict__ partial) {
  __shared__ float red[256];
  const int s = blockIdx.y;
  const int64_t off = seg_off[s], len = seg_len[s];
  const int64_t c0 = (int64_t)blockIdx.x * kNormChunk;
  const int64_t c1 = c0 + kNormChunk < len ? c0 + kNormChunk : len;
  float acc = 0.f;
  for (int64_t i = c0 + threadIdx.x; i < c1; i += 256) acc = fmaf(v[off + i], v[off + i], acc);
  const float sum = block_sum(acc, red);
  if (threadIdx.x == 0) partial[(int64_t)s * n_chunks + blockIdx.x] = sum;
}

__global__ __launch_bounds__(256) void k_seg_norm_final(int n_chunks, const float* __restrict__ partial,
                                                        float* __restrict__ norms) {
  __shared__ float red[256];
  const float* p = partial + (int64_t)blockIdx.x * n_chunks;
  float acc = 0.f;
  for (int c = threadIdx.x; c < n_chunks; c += 256) acc += p[c];
  const float sum = block_sum(acc, red);
  if (threadIdx.x == 0) norms[blockIdx.x] = sqrtf(sum);
}

__global__ void k_gather(int T, int B, int D, const float* __restrict__ pool, const int64_t* __restrict__ row0,
                         const int32_t* __restrict__ len, float* __restrict__ X0) {
  const int64_t total = (int64_t)T * B * D;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int d = (int)(i % D);
    const int64_t tb = i / D;
    const int b = (int)(tb % B), t = (int)(tb / B);
    X0[i] = (t >= 1 && t < len[b]) ? pool[(row0[b] + t - 1) * D + d] : 0.f;
  }
}

__global__ void k_transpose(int64_t rows, int64_t cols, const float* __restrict__ W, float* __restrict__ WT) {
  const int64_t total = rows * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cols, c = i % cols;
    WT[c * rows + r] = W[i];
  }
}

// Hs[0][b] = rnn_init_hidden[layer] for every column b.
__global__ void k_init_hidden(int B, int H, const float* __restrict__ h0, float* __restrict__ Hs) {
  const int64_t total = (int64_t)B * H;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
    Hs[i] = h0[i % H];
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// One forward step t of a GRU layer.  Workgroup (b, unit block): h_{t-1}[b] is staged in LDS in chunks.
// Hs holds T+1 states per column (Hs[0] = rnn_init_hidden); a column past its length keeps its state.
__global__ __launch_bounds__(256) void k_gru_fwd_step(int t, int B, int H, const int32_t* __restrict__ len,
                                                      const float* __restrict__ Gi, const float* __restrict__ WT,
                                                      const float* __restrict__ bhh, float* __restrict__ Hs,
                                                      float* __restrict__ R, float* __restrict__ Z,
                                                      float* __restrict__ Nn, float* __restrict__ GHN,
                                                      float* __restrict__ Y) {
  __shared__ float hs[kChunk];
  const int b = blockIdx.x;
  const int j = blockIdx.y * 256 + threadIdx.x;
  const int64_t H3 = 3 * (int64_t)H;
  const float* hprev = Hs + ((int64_t)t * B + b) * H;
  float* hnext = Hs + ((int64_t)(t + 1) * B + b) * H;
  const int64_t row = (int64_t)t * B + b;
  if (t >= len[b]) {  // block-uniform
    if (j < H) {
      hnext[j] = hprev[j];
      Y[row * H + j] = 0.f;
      R[row * H + j] = 0.f; Z[row * H + j] = 0.f; Nn[row * H + j] = 0.f; GHN[row * H + j] = 0.f;
    }
    return;
  }
  float ar = 0.f, az = 0.f, an = 0.f;
  for (int k0 = 0; k0 < H; k0 += kChunk) {
    const int kn = min(kChunk, H - k0);
    __syncthreads();
    for (int k = threadIdx.x; k < kn; k += 256) hs[k] = hprev[k0 + k];
    __syncthreads();
    if (j < H) {
      const float* w = WT + (int64_t)k0 * H3 + j;
      for (int k = 0; k < kn; ++k) {
        const float hk = hs[k];
        ar = fmaf(hk, w[0], ar);
        az = fmaf(hk, w[H], az);
        an = fmaf(hk, w[2 * (int64_t)H], an);
        w += H3;
      }
    }
  }
  if (j >= H) return;
  const float* gi = Gi + row * H3;
  const float ghn = an + bhh[2 * H + j];
  const float r = sigmoidf_(gi[j] + (ar + bhh[j]));
  const float z = sigmoidf_(gi[H + j] + (az + bhh[H + j]));
  const float n = tanhf(gi[2 * H + j] + r * ghn);
  const float hp = hprev[j];
  const float h = n + z * (hp - n);
  hnext[j] = h;
  Y[row * H + j] = h;
  R[row * H + j] = r; Z[row * H + j] = z; Nn[row * H + j] = n; GHN[row * H + j] = ghn;
}

// One reverse step t of a GRU layer.  Workgroup (b, unit block), thread = unit k:
//   dh_t = dY[t] + dh_{t+1} ⊙ z_{t+1} + Σ_j dGh_{t+1}[j] W_hh[j, k]
// then the gate gradients of step t.  t == -1: dh_{-1} only (into dH0, the rnn_init_hidden part).
__global__ __launch_bounds__(256) void k_gru_bwd_step(int t, int T, int B, int H, const int32_t* __restrict__ len,
                                                      const float* __restrict__ W, const float* __restrict__ dY,
                                                      const float* __restrict__ R, const float* __restrict__ Z,
                                                      const float* __restrict__ Nn, const float* __restrict__ GHN,
                                                      const float* __restrict__ Hs, float* __restrict__ dGi,
                                                      float* __restrict__ dGh, float* __restrict__ dHZ,
                                                      float* __restrict__ dH0) {
  __shared__ float gs[kChunk];
  const int b = blockIdx.x;
  const int k = blockIdx.y * 256 + threadIdx.x;
  const int64_t H3 = 3 * (int64_t)H;
  float carry = 0.f;
  if (t + 1 < T) {  // block-uniform
    const int64_t nrow = (int64_t)(t + 1) * B + b;
    const float* g = dGh + nrow * H3;
    for (int64_t j0 = 0; j0 < H3; j0 += kChunk) {
      const int jn = (int)min((int64_t)kChunk, H3 - j0);
      __syncthreads();
      for (int j = threadIdx.x; j < jn; j += 256) gs[j] = g[j0 + j];
      __syncthreads();
      if (k < H) {
        const float* w = W + j0 * H + k;
        for (int j = 0; j < jn; ++j) {
          carry = fmaf(gs[j], w[0], carry);
          w += H;
        }
      }
    }
    if (k < H) carry += dHZ[nrow * H + k];
  }
  if (k >= H) return;
  if (t < 0) {
    dH0[(int64_t)b * H + k] = carry;
    return;
  }
  const int64_t row = (int64_t)t * B + b;
  float* dgi = dGi + row * H3;
  float* dgh = dGh + row * H3;
  if (t >= len[b]) {  // past this column's length: no state, no gradient (the carry is 0 here)
    dgi[k] = 0.f; dgi[H + k] = 0.f; dgi[2 * H + k] = 0.f;
    dgh[k] = 0.f; dgh[H + k] = 0.f; dgh[2 * H + k] = 0.f;
    dHZ[row * H + k] = 0.f;
    return;
  }
  const float dh = dY[row * H + k] + carry;
  const float r = R[row * H + k], z = Z[row * H + k], n = Nn[row * H + k], ghn = GHN[row * H + k];
  const float hp = Hs[row * H + k];  // h_{t-1}
  const float dn = dh * (1.f - z);
  const float dz = dh * (hp - n);
  const float dnp = dn * (1.f - n * n);
  const float dr = dnp * ghn;
  const float drp = dr * (r * (1.f - r));
  const float dzp = dz * (z * (1.f - z));
  dgi[k] = drp; dgi[H + k] = dzp; dgi[2 * H + k] = dnp;
  dgh[k] = drp; dgh[H + k] = dzp; dgh[2 * H + k] = dnp * r;
  dHZ[row * H + k] = dh * z;
}

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

// Inter-layer dropout (train mode): keep with probability 1-p and scale by 1/(1-p).  The mask is a
// counter-based hash of (key, iteration, layer, element): the backward pass recomputes it.
__device__ __forceinline__ float dropout_scale(uint64_t key, uint64_t iter, int layer, int64_t i, float p) {
  if (p <= 0.f) return 1.f;
  if (p >= 1.f) return 0.f;
  const uint64_t h = mix64(key ^ mix64(iter * 0x100000001b3ull + (uint64_t)layer) ^ mix64((uint64_t)i));
  const float u = (float)(h >> 40) * (1.f / 16777216.f);
  return u >= p ? 1.f / (1.f - p) : 0.f;
}

__global__ void k_dropout(int64_t n, const float* __restrict__ in, float* __restrict__ out, uint64_t key,
                          uint64_t iter, int layer, float p) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = in[i] * dropout_scale(key, iter, layer, i, p);
}

// torch's relu keeps NaN; its backward passes the gradient where the output is > 0.
__global__ void k_relu(int64_t n, const float* __restrict__ in, float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float x = in[i];
    out[i] = (x > 0.f || x != x) ? x : 0.f;
  }
}

__global__ void k_relu_bwd(int64_t n, const float* __restrict__ out, float* __restrict__ g) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    if (!(out[i] > 0.f)) g[i] = 0.f;
}

// Thread (b, d): cumsum of mean over time, / (t+1), and the masked difference to the truth X0[t+1].
__global__ void k_loss_rows(int T, int B, int D, const float* __restrict__ M, const float* __restrict__ X0,
                            float* __restrict__ diff) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)B * D;
       i += (int64_t)gridDim.x * blockDim.x) {
  float c = 0.f;
  for (int t = 0; t + 1 < T; ++t) {
    c += M[(int64_t)t * B * D + i];
    const float mean = c * (1.f / (float)(t + 1));
    const float tr = X0[(int64_t)(t + 1) * B * D + i];
    diff[(int64_t)t * B * D + i] = (tr != 0.f ? 1.f : 0.f) * mean - tr;
  }
  }
}

// Workgroup d: S_d = Σ diff², n_d = #(diff² != 0) over the (T-1)·B rows.
__global__ __launch_bounds__(256) void k_colstats(int64_t rows, int D, const float* __restrict__ diff,
                                                  float* __restrict__ S, float* __restrict__ Ncnt) {
  __shared__ float red[256];
  const int d = blockIdx.x;
  float s = 0.f, c = 0.f;
  for (int64_t r = threadIdx.x; r < rows; r += 256) {
    const float x = diff[r * D + d];
    const float sq = x * x;
    s += sq;
    c += (sq != 0.f) ? 1.f : 0.f;
  }
  const float ss = block_sum(s, red);
  __syncthreads();
  const float cc = block_sum(c, red);
  if (threadIdx.x == 0) { S[d] = ss; Ncnt[d] = cc; }
}

struct LossConsts {
  float sigma_alpha, sigma_beta, reg;
  int n_rnn_seg;
};

// One workgroup: the three losses and the sigma2 gradient (loss1 + loss2).
__global__ __launch_bounds__(256) void k_losses(int D, LossConsts lc, const float* __restrict__ S,
                                                const float* __restrict__ Ncnt, const float* __restrict__ sigma2,
                                                const float* __restrict__ pnorms, float* __restrict__ dsigma2,
                                                float* __restrict__ losses) {
  __shared__ float red[256];
  const float nz = Ncnt[0];
  float l1 = 0.f, l2 = 0.f;
  for (int d = threadIdx.x; d < D; d += 256) {
    const float s2 = sigma2[d], nd = Ncnt[d];
    const float w = 1.f / (2.f * s2);
    l1 += S[d] * w;
    const float a = (2.f * lc.sigma_alpha + nd + 2.f) / (2.f * nd);
    l2 += a * logf(s2) + lc.sigma_beta / (s2 * nd);
    dsigma2[d] = -S[d] / (2.f * s2 * s2) / nz + a / s2 - lc.sigma_beta / (nd * s2 * s2);
  }
  const float L1 = block_sum(l1, red) / nz;
  __syncthreads();
  const float L2 = block_sum(l2, red);
  if (threadIdx.x == 0) {
    float sn = 0.f;
    for (int s = 0; s < lc.n_rnn_seg; ++s) sn += pnorms[s];
    const float L3 = lc.reg * sn;
    losses[0] = (L1 + L2) + L3;
    losses[1] = L1;
    losses[2] = L2;
    losses[3] = L3;
  }
}

// Thread (b, d): d mean = mask · 2 diff w_d / nz, then the reverse cumsum with the 1/(t+1) factor.
__global__ void k_dmean(int T, int B, int D, const float* __restrict__ X0, const float* __restrict__ diff,
                        const float* __restrict__ sigma2, const float* __restrict__ Ncnt, float* __restrict__ dM) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)B * D;
       i += (int64_t)gridDim.x * blockDim.x) {
  const int d = (int)(i % D);
  const float g = (1.f / (2.f * sigma2[d])) / Ncnt[0];
  float acc = 0.f;
  for (int t = T - 1; t >= 0; --t) {
    if (t + 1 < T) {
      const float tr = X0[(int64_t)(t + 1) * B * D + i];
      const float dmean = (tr != 0.f ? 1.f : 0.f) * (2.f * diff[(int64_t)t * B * D + i] * g);
      acc += dmean * (1.f / (float)(t + 1));
    }
    dM[(int64_t)t * B * D + i] = acc;
  }
  }
}

// grad += reg · p / ‖p‖ over the CoreRNN segments (torch's norm backward gives 0 at ‖p‖ = 0).
__global__ void k_reg_grad(const float* __restrict__ P, float* __restrict__ G, const int64_t* __restrict__ seg_off,
                           const int64_t* __restrict__ seg_len, const float* __restrict__ pnorms, float reg) {
  const int s = blockIdx.y;
  const int64_t off = seg_off[s], len = seg_len[s];
  const float nrm = pnorms[s];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (int64_t)gridDim.x * blockDim.x) {
    const float q = nrm != 0.f ? P[off + i] / nrm : 0.f;
    G[off + i] += reg * q;
  }
}

struct AdamConsts {
  float lr_over_bc1, bc2_sqrt, max_norm;
  int n_rnn_seg;
  int64_t n_rnn, n_adam, sigma_off, sigma_len;
};

// clip_grad_norm_ over [0, n_rnn), Adam over [0, n_adam), then sigma2 >= 1e-6 -- torch's arithmetic order.
__global__ void k_clip_adam(AdamConsts ac, const float* __restrict__ gnorms, float* __restrict__ P,
                            float* __restrict__ G, float* __restrict__ Mo, float* __restrict__ Vo) {
  float tot = 0.f;
  for (int s = 0; s < ac.n_rnn_seg; ++s) tot += gnorms[s] * gnorms[s];
  tot = sqrtf(tot);
  float coef = ac.max_norm / (tot + 1e-6f);
  coef = coef < 1.f ? coef : 1.f;
  const int64_t n = ac.sigma_off + ac.sigma_len;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float p = P[i];
    if (i < ac.n_adam) {
      float g = G[i];
      if (i < ac.n_rnn) {
        g *= coef;
        G[i] = g;
      }
      const float m = Mo[i] + 0.1f * (g - Mo[i]);
      const float v = Vo[i] * 0.999f + 0.001f * (g * g);
      Mo[i] = m;
      Vo[i] = v;
      const float denom = sqrtf(v) / ac.bc2_sqrt + 1e-8f;
      p = p + (-ac.lr_over_bc1) * (m / denom);
    }
    if (i >= ac.sigma_off) p = (p < 1e-6f) ? 1e-6f : p;
    P[i] = p;
  }
}

int grid1(int64_t n, int block = 256) {
  int64_t g = (n + block - 1) / block;
  if (g < 1) g = 1;
  if (g > 65536) g = 65536;
  return (int)g;
}

}  // namespace

struct uis_trainer {
  int device = 0;
  int D = 0, H = 0, L = 0;
  uis_train_opts opts{};
  hipStream_t stream = nullptr;
  // flat parameters / gradients / Adam moments
  int64_t n_total = 0, n_rnn = 0, n_adam = 0;
  std::vector<int64_t> seg_off, seg_len;  // CoreRNN segments, then rnn_init_hidden, then sigma2
  int n_rnn_seg = 0;
  float *P = nullptr, *G = nullptr, *Mo = nullptr, *Vo = nullptr;
  int64_t *d_seg_off = nullptr, *d_seg_len = nullptr;
  float *pnorms = nullptr, *gnorms = nullptr, *losses = nullptr;
  float* norm_partial = nullptr;  // [n_rnn_seg, norm_chunks] (k_seg_sq_partial)
  int norm_chunks = 0;
  int64_t adam_step = 0;
  uint64_t iter = 0;
  // data
  float* pool = nullptr;
  std::vector<int64_t> seq_off;
  int n_seqs = 0;
  int64_t *d_row0 = nullptr;
  int32_t* d_len = nullptr;
  // pinned host staging of each step's batch (the H2D copies are asynchronous); `staged` marks
  // when the stream has consumed them, so the next step waits on it before overwriting them
  int64_t* h_row0 = nullptr;
  int32_t* h_len = nullptr;
  hipEvent_t staged = nullptr;
  bool staged_pending = false;
  int cap_B = 0;
  // workspace (sized for cap_TB rows)
  int64_t cap_TB = 0;
  float* ws = nullptr;

  int64_t w_ih(int l) const { return seg_off[4 * l]; }
  int64_t w_hh(int l) const { return seg_off[4 * l + 1]; }
  int64_t b_ih(int l) const { return seg_off[4 * l + 2]; }
  int64_t b_hh(int l) const { return seg_off[4 * l + 3]; }
  int64_t w1() const { return seg_off[4 * L]; }
  int64_t b1() const { return seg_off[4 * L + 1]; }
  int64_t w2() const { return seg_off[4 * L + 2]; }
  int64_t b2() const { return seg_off[4 * L + 3]; }
  int64_t h0() const { return seg_off[4 * L + 4]; }
  int64_t s2() const { return seg_off[4 * L + 5]; }
  int in_dim(int l) const { return l == 0 ? D : H; }
};

namespace {

void free_all(uis_trainer* th) {
  for (void* p : {(void*)th->P, (void*)th->G, (void*)th->Mo, (void*)th->Vo, (void*)th->d_seg_off,
                  (void*)th->d_seg_len, (void*)th->pnorms, (void*)th->gnorms, (void*)th->losses,
                  (void*)th->pool, (void*)th->d_row0, (void*)th->d_len, (void*)th->ws,
                  (void*)th->norm_partial})
    if (p) (void)hipFree(p);
  if (th->h_row0) (void)hipHostFree(th->h_row0);
  if (th->h_len) (void)hipHostFree(th->h_len);
  if (th->staged) (void)hipEventDestroy(th->staged);
  if (th->stream) (void)hipStreamDestroy(th->stream);
}

// Workspace layout for T·B rows (floats).  Per layer: X (input, layers >= 1), Gi, Hs, R, Z, N, GHN, Y.
struct Ws {
  float* X0;
  std::vector<float*> X, Gi, Hs, R, Z, Nn, GHN, Y;
  float *A1, *Rl, *M, *diff, *dM, *dR, *dY, *dGi, *dGh, *dHZ, *dH0, *S, *Ncnt;
};

int64_t ws_floats(const uis_trainer* th, int64_t TB, int64_t B, Ws* w, float* base) {
  const int64_t D = th->D, H = th->H;
  int64_t off = 0;
  auto take = [&](int64_t n) {
    float* p = base ? base + off : nullptr;
    off += (n + 63) / 64 * 64;
    return p;
  };
  if (w) {
    w->X.assign(th->L, nullptr); w->Gi = w->X; w->Hs = w->X; w->R = w->X; w->Z = w->X;
    w->Nn = w->X; w->GHN = w->X; w->Y = w->X;
  }
  float* p;
  p = take(TB * D); if (w) w->X0 = p;
  for (int l = 0; l < th->L; ++l) {
    p = l ? take(TB * H) : nullptr; if (w) w->X[l] = l ? p : w->X0;
    p = take(TB * 3 * H); if (w) w->Gi[l] = p;
    p = take(TB * H + B * H); if (w) w->Hs[l] = p;
    p = take(TB * H); if (w) w->R[l] = p;
    p = take(TB * H); if (w) w->Z[l] = p;
    p = take(TB * H); if (w) w->Nn[l] = p;
    p = take(TB * H); if (w) w->GHN[l] = p;
    p = take(TB * H); if (w) w->Y[l] = p;
  }
  p = take(TB * H); if (w) w->A1 = p;
  p = take(TB * H); if (w) w->Rl = p;
  p = take(TB * D); if (w) w->M = p;
  p = take(TB * D); if (w) w->diff = p;
  p = take(TB * D); if (w) w->dM = p;
  p = take(TB * H); if (w) w->dR = p;
  p = take(TB * std::max<int64_t>(H, D)); if (w) w->dY = p;
  p = take(TB * 3 * H); if (w) w->dGi = p;
  p = take(TB * 3 * H); if (w) w->dGh = p;
  p = take(TB * H); if (w) w->dHZ = p;
  p = take(B * H); if (w) w->dH0 = p;
  p = take(D); if (w) w->S = p;
  p = take(D); if (w) w->Ncnt = p;
  p = take(3 * H * H); (void)p;  // W_hhᵀ of the layer being run forward
  return off;
}

void gemm(hipStream_t st, int64_t M, int64_t N, int64_t K, const float* A, int64_t sam, int64_t sak,
          const float* B, int64_t sbk, int64_t sbn, float* C, int64_t ldc, const float* bias) {
  dim3 grid((unsigned)((M + kTile - 1) / kTile), (unsigned)((N + kTile - 1) / kTile));
  hipLaunchKernelGGL(k_gemm, grid, dim3(256), 0, st, M, N, K, A, sam, sak, B, sbk, sbn, C, ldc, bias);
}

// Norms of the CoreRNN segments of the flat vector v (parameters or gradients).
void seg_norms(const uis_trainer* th, const float* v, float* norms) {
  hipLaunchKernelGGL(k_seg_sq_partial, dim3((unsigned)th->norm_chunks, (unsigned)th->n_rnn_seg), dim3(256), 0,
                     th->stream, v, th->d_seg_off, th->d_seg_len, th->norm_chunks, th->norm_partial);
  hipLaunchKernelGGL(k_seg_norm_final, dim3((unsigned)th->n_rnn_seg), dim3(256), 0, th->stream, th->norm_chunks,
                     th->norm_partial, norms);
}

void colsum(hipStream_t st, int64_t rows, int64_t cols, const float* X, float* out) {
  hipLaunchKernelGGL(k_colsum, dim3((unsigned)((cols + 63) / 64)), dim3(256), 0, st, rows, cols, X, out);
}

}  // namespace

UIS_EXPORT int32_t uis_train_create(const uis_model_desc* desc, const uis_train_opts* opts, int32_t device,
                                    uis_trainer** out) {
  if (!desc || !opts || !out) return tfail(UIS_ERR_INVALID_ARG, "uis_train_create: NULL argument");
  *out = nullptr;
  const int D = desc->observation_dim, H = desc->rnn_hidden_size, L = desc->rnn_depth;
  if (D <= 0 || H <= 0 || L <= 0)
    return tfail(UIS_ERR_INVALID_ARG, "uis_train_create: observation_dim, rnn_hidden_size and rnn_depth must be positive");
  if (!desc->gru_weight_ih || !desc->gru_weight_hh || !desc->gru_bias_ih || !desc->gru_bias_hh ||
      !desc->linear_mean1_weight || !desc->linear_mean1_bias || !desc->linear_mean2_weight ||
      !desc->linear_mean2_bias || !desc->rnn_init_hidden || !desc->sigma2)
    return tfail(UIS_ERR_INVALID_ARG, "uis_train_create: NULL weight pointer");
  for (int l = 0; l < L; ++l)
    if (!desc->gru_weight_ih[l] || !desc->gru_weight_hh[l] || !desc->gru_bias_ih[l] || !desc->gru_bias_hh[l])
      return tfail(UIS_ERR_INVALID_ARG, "uis_train_create: NULL weight pointer");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return tfail(UIS_ERR_NO_DEVICE, "no HIP device visible; the trainer has no CPU fallback");
  if (device < 0 || device >= ndev) return tfail(UIS_ERR_NO_DEVICE, "device index out of range");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return tfail(UIS_ERR_NO_DEVICE, "hipGetDeviceProperties failed");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return tfail(UIS_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
  TCHK(hipSetDevice(device));

  uis_trainer* th = new uis_trainer();
  th->device = device;
  th->D = D; th->H = H; th->L = L;
  th->opts = *opts;
  std::vector<const float*> src;
  auto add = [&](const float* p, int64_t n) {
    th->seg_off.push_back(th->n_total);
    th->seg_len.push_back(n);
    src.push_back(p);
    th->n_total += n;
  };
  for (int l = 0; l < L; ++l) {
    add(desc->gru_weight_ih[l], 3LL * H * th->in_dim(l));
    add(desc->gru_weight_hh[l], 3LL * H * H);
    add(desc->gru_bias_ih[l], 3LL * H);
    add(desc->gru_bias_hh[l], 3LL * H);
  }
  add(desc->linear_mean1_weight, (int64_t)H * H);
  add(desc->linear_mean1_bias, H);
  add(desc->linear_mean2_weight, (int64_t)D * H);
  add(desc->linear_mean2_bias, D);
  th->n_rnn_seg = 4 * L + 4;
  th->n_rnn = th->n_total;
  add(desc->rnn_init_hidden, (int64_t)L * H);
  add(desc->sigma2, D);
  th->n_adam = opts->estimate_sigma2 ? th->n_total : th->s2();

  auto fail_free = [&](int rc) { free_all(th); delete th; return rc; };
  hipError_t e = hipStreamCreateWithFlags(&th->stream, hipStreamNonBlocking);
  const size_t bytes = sizeof(float) * (size_t)th->n_total;
  const size_t nseg = th->seg_off.size();
  if (e == hipSuccess) e = hipMalloc(&th->P, bytes);
  if (e == hipSuccess) e = hipMalloc(&th->G, bytes);
  if (e == hipSuccess) e = hipMalloc(&th->Mo, bytes);
  if (e == hipSuccess) e = hipMalloc(&th->Vo, bytes);
  if (e == hipSuccess) e = hipMalloc(&th->d_seg_off, nseg * sizeof(int64_t));
  if (e == hipSuccess) e = hipMalloc(&th->d_seg_len, nseg * sizeof(int64_t));
  if (e == hipSuccess) e = hipMalloc(&th->pnorms, nseg * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&th->gnorms, nseg * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&th->losses, 4 * sizeof(float));
  if (e == hipSuccess) e = hipEventCreateWithFlags(&th->staged, hipEventDisableTiming);
  {
    int64_t maxlen = 0;
    for (int s = 0; s < th->n_rnn_seg; ++s) maxlen = std::max(maxlen, th->seg_len[s]);
    th->norm_chunks = (int)((maxlen + kNormChunk - 1) / kNormChunk);
  }
  if (e == hipSuccess) e = hipMalloc(&th->norm_partial, sizeof(float) * (size_t)th->n_rnn_seg * th->norm_chunks);
  if (e == hipSuccess) e = hipMemsetAsync(th->G, 0, bytes, th->stream);
  if (e == hipSuccess) e = hipMemsetAsync(th->Mo, 0, bytes, th->stream);
  if (e == hipSuccess) e = hipMemsetAsync(th->Vo, 0, bytes, th->stream);
  for (size_t s = 0; s < nseg && e == hipSuccess; ++s)
    e = hipMemcpyAsync(th->P + th->seg_off[s], src[s], th->seg_len[s] * sizeof(float), hipMemcpyHostToDevice,
                       th->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(th->d_seg_off, th->seg_off.data(), nseg * sizeof(int64_t), hipMemcpyHostToDevice, th->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(th->d_seg_len, th->seg_len.data(), nseg * sizeof(int64_t), hipMemcpyHostToDevice, th->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(th->stream);
  if (e != hipSuccess)
    return fail_free(tfail(e == hipErrorOutOfMemory ? UIS_ERR_OOM : UIS_ERR_HIP,
                           std::string("uis_train_create: ") + hipGetErrorString(e)));
  *out = th;
  return UIS_OK;
}

UIS_EXPORT int32_t uis_train_set_data(uis_trainer* th, const float* pool, const int64_t* seq_offsets, int32_t n_seqs) {
  if (!th || !pool || !seq_offsets) return tfail(UIS_ERR_INVALID_ARG, "uis_train_set_data: NULL argument");
  if (n_seqs <= 0) return tfail(UIS_ERR_INVALID_ARG, "uis_train_set_data: n_seqs must be positive");
  if (seq_offsets[0] != 0) return tfail(UIS_ERR_INVALID_ARG, "uis_train_set_data: seq_offsets[0] must be 0");
  for (int s = 0; s < n_seqs; ++s)
    if (seq_offsets[s + 1] <= seq_offsets[s])
      return tfail(UIS_ERR_INVALID_ARG, "uis_train_set_data: every sub-sequence needs at least one row");
  if (seq_offsets[n_seqs] >= INT32_MAX)
    return tfail(UIS_ERR_UNSUPPORTED, "uis_train_set_data: more than 2^31 rows");
  TCHK(hipSetDevice(th->device));
  TCHK(hipStreamSynchronize(th->stream));
  if (th->pool) { TCHK(hipFree(th->pool)); th->pool = nullptr; }
  const size_t bytes = sizeof(float) * (size_t)seq_offsets[n_seqs] * th->D;
  TCHK(hipMalloc(&th->pool, bytes));
  TCHK(hipMemcpy(th->pool, pool, bytes, hipMemcpyHostToDevice));
  th->seq_off.assign(seq_offsets, seq_offsets + n_seqs + 1);
  th->n_seqs = n_seqs;
  return UIS_OK;
}

UIS_EXPORT int32_t uis_train_step(uis_trainer* th, const int32_t* batch_idx, int32_t batch_size, float* out_losses) {
  if (!th || !batch_idx) return tfail(UIS_ERR_INVALID_ARG, "uis_train_step: NULL argument");
  if (!th->pool) return tfail(UIS_ERR_INVALID_ARG, "uis_train_step: no data (uis_train_set_data)");
  if (batch_size <= 0) return tfail(UIS_ERR_INVALID_ARG, "uis_train_step: batch_size must be positive");
  const int B = batch_size, D = th->D, H = th->H, L = th->L;
  std::vector<int64_t> row0(B);
  std::vector<int32_t> len(B);
  for (int b = 0; b < B; ++b) {
    const int s = batch_idx[b];
    if (s < 0 || s >= th->n_seqs) return tfail(UIS_ERR_INVALID_ARG, "uis_train_step: batch index out of range");
    row0[b] = th->seq_off[s];
    len[b] = (int32_t)(th->seq_off[s + 1] - th->seq_off[s] + 1);  // the reference's seq_lengths: rows + 1
    if (b && len[b] > len[b - 1])
      return tfail(UIS_ERR_INVALID_ARG, "uis_train_step: the batch's sub-sequences must be in non-increasing length order");
  }
  const int T = len[0];
  const int64_t TB = (int64_t)T * B;
  hipStream_t st = th->stream;
  TCHK(hipSetDevice(th->device));

  // device buffers that grow with the batch
  if (B > th->cap_B) {
    TCHK(hipStreamSynchronize(st));
    if (th->d_row0) { TCHK(hipFree(th->d_row0)); th->d_row0 = nullptr; }
    if (th->d_len) { TCHK(hipFree(th->d_len)); th->d_len = nullptr; }
    if (th->h_row0) { TCHK(hipHostFree(th->h_row0)); th->h_row0 = nullptr; }
    if (th->h_len) { TCHK(hipHostFree(th->h_len)); th->h_len = nullptr; }
    th->staged_pending = false;  // (the stream was synchronised above)
    TCHK(hipMalloc(&th->d_row0, sizeof(int64_t) * B));
    TCHK(hipMalloc(&th->d_len, sizeof(int32_t) * B));
    TCHK(hipHostMalloc((void**)&th->h_row0, sizeof(int64_t) * B, hipHostMallocDefault));
    TCHK(hipHostMalloc((void**)&th->h_len, sizeof(int32_t) * B, hipHostMallocDefault));
    th->cap_B = B;
    th->cap_TB = 0;  // the workspace's B-sized parts grow too
  }
  if (TB > th->cap_TB) {
    TCHK(hipStreamSynchronize(st));
    if (th->ws) { TCHK(hipFree(th->ws)); th->ws = nullptr; }
    const int64_t cap = std::max<int64_t>(TB, (int64_t)T * th->cap_B);
    TCHK(hipMalloc(&th->ws, sizeof(float) * (size_t)ws_floats(th, cap, th->cap_B, nullptr, nullptr)));
    th->cap_TB = cap;
  }
  {  // UIS_POISON_WORKSPACE: the whole workspace, on the trainer's stream ahead of the step's first kernel
    const UisPoison poison = UisPoison::from_env();
    if (poison.on)
      TCHK(poison.device(th->ws, sizeof(float) * (size_t)ws_floats(th, th->cap_TB, th->cap_B, nullptr, nullptr), st));
  }
  Ws w;
  const int64_t wsn = ws_floats(th, TB, B, &w, th->ws);
  float* WT = th->ws + wsn - (3LL * H * H + 63) / 64 * 64;
  // the previous step's copies must have left the staging buffers before they are rewritten
  if (th->staged_pending) TCHK(hipEventSynchronize(th->staged));
  std::memcpy(th->h_row0, row0.data(), sizeof(int64_t) * B);
  std::memcpy(th->h_len, len.data(), sizeof(int32_t) * B);
  TCHK(hipMemcpyAsync(th->d_row0, th->h_row0, sizeof(int64_t) * B, hipMemcpyHostToDevice, st));
  TCHK(hipMemcpyAsync(th->d_len, th->h_len, sizeof(int32_t) * B, hipMemcpyHostToDevice, st));
  TCHK(hipEventRecord(th->staged, st));
  th->staged_pending = true;

  float* P = th->P;
  float* G = th->G;
  const float p_drop = L >= 2 ? (float)th->opts.dropout : 0.f;
  const uint64_t key = th->opts.dropout_key, iter = th->iter;
  const dim3 step_grid((unsigned)B, (unsigned)((H + 255) / 256));

  // ---- forward
  hipLaunchKernelGGL(k_gather, dim3(grid1(TB * D)), dim3(256), 0, st, T, B, D, th->pool, th->d_row0, th->d_len, w.X0);
  for (int l = 0; l < L; ++l) {
    const int Din = th->in_dim(l);
    if (l > 0)
      hipLaunchKernelGGL(k_dropout, dim3(grid1(TB * H)), dim3(256), 0, st, TB * H, w.Y[l - 1], w.X[l], key, iter, l,
                         p_drop);
    gemm(st, TB, 3LL * H, Din, w.X[l], Din, 1, P + th->w_ih(l), 1, Din, w.Gi[l], 3LL * H, P + th->b_ih(l));
    hipLaunchKernelGGL(k_transpose, dim3(grid1(3LL * H * H)), dim3(256), 0, st, 3LL * H, (int64_t)H,
                       P + th->w_hh(l), WT);
    hipLaunchKernelGGL(k_init_hidden, dim3(grid1((int64_t)B * H)), dim3(256), 0, st, B, H,
                       P + th->h0() + (int64_t)l * H, w.Hs[l]);
    for (int t = 0; t < T; ++t)
      hipLaunchKernelGGL(k_gru_fwd_step, step_grid, dim3(256), 0, st, t, B, H, th->d_len, w.Gi[l], WT,
                         P + th->b_hh(l), w.Hs[l], w.R[l], w.Z[l], w.Nn[l], w.GHN[l], w.Y[l]);
  }
  gemm(st, TB, H, H, w.Y[L - 1], H, 1, P + th->w1(), 1, H, w.A1, H, P + th->b1());
  hipLaunchKernelGGL(k_relu, dim3(grid1(TB * H)), dim3(256), 0, st, TB * H, w.A1, w.Rl);
  gemm(st, TB, D, H, w.Rl, H, 1, P + th->w2(), 1, H, w.M, D, P + th->b2());

  // ---- losses
  const int64_t BD = (int64_t)B * D;
  hipLaunchKernelGGL(k_loss_rows, dim3(grid1(BD)), dim3(256), 0, st, T, B, D, w.M, w.X0, w.diff);
  hipLaunchKernelGGL(k_colstats, dim3(D), dim3(256), 0, st, (int64_t)(T - 1) * B, D, w.diff, w.S, w.Ncnt);
  seg_norms(th, P, th->pnorms);
  LossConsts lc{(float)th->opts.sigma_alpha, (float)th->opts.sigma_beta, (float)th->opts.regularization_weight,
                th->n_rnn_seg};
  hipLaunchKernelGGL(k_losses, dim3(1), dim3(256), 0, st, D, lc, w.S, w.Ncnt, P + th->s2(), th->pnorms,
                     G + th->s2(), th->losses);

  // ---- backward: head
  hipLaunchKernelGGL(k_dmean, dim3(grid1(BD)), dim3(256), 0, st, T, B, D, w.X0, w.diff, P + th->s2(), w.Ncnt, w.dM);
  colsum(st, TB, D, w.dM, G + th->b2());
  gemm(st, D, H, TB, w.dM, 1, D, w.Rl, H, 1, G + th->w2(), H, nullptr);
  gemm(st, TB, H, D, w.dM, D, 1, P + th->w2(), H, 1, w.dR, H, nullptr);
  hipLaunchKernelGGL(k_relu_bwd, dim3(grid1(TB * H)), dim3(256), 0, st, TB * H, w.A1, w.dR);
  colsum(st, TB, H, w.dR, G + th->b1());
  gemm(st, H, H, TB, w.dR, 1, H, w.Y[L - 1], H, 1, G + th->w1(), H, nullptr);
  gemm(st, TB, H, H, w.dR, H, 1, P + th->w1(), H, 1, w.dY, H, nullptr);

  // ---- backward: GRU layers, last to first
  for (int l = L - 1; l >= 0; --l) {
    const int Din = th->in_dim(l);
    for (int t = T - 1; t >= -1; --t)
      hipLaunchKernelGGL(k_gru_bwd_step, step_grid, dim3(256), 0, st, t, T, B, H, th->d_len, P + th->w_hh(l), w.dY,
                         w.R[l], w.Z[l], w.Nn[l], w.GHN[l], w.Hs[l], w.dGi, w.dGh, w.dHZ, w.dH0);
    gemm(st, 3LL * H, Din, TB, w.dGi, 1, 3LL * H, w.X[l], Din, 1, G + th->w_ih(l), Din, nullptr);
    gemm(st, 3LL * H, H, TB, w.dGh, 1, 3LL * H, w.Hs[l], H, 1, G + th->w_hh(l), H, nullptr);
    colsum(st, TB, 3LL * H, w.dGi, G + th->b_ih(l));
    colsum(st, TB, 3LL * H, w.dGh, G + th->b_hh(l));
    colsum(st, B, H, w.dH0, G + th->h0() + (int64_t)l * H);
    if (l > 0) {
      gemm(st, TB, H, 3LL * H, w.dGi, 3LL * H, 1, P + th->w_ih(l), H, 1, w.dR, H, nullptr);
      hipLaunchKernelGGL(k_dropout, dim3(grid1(TB * H)), dim3(256), 0, st, TB * H, w.dR, w.dY, key, iter, l, p_drop);
    }
  }

  // ---- regularisation gradient, clip, Adam
  {
    int64_t maxlen = 0;
    for (int s = 0; s < th->n_rnn_seg; ++s) maxlen = std::max(maxlen, th->seg_len[s]);
    hipLaunchKernelGGL(k_reg_grad, dim3(grid1(maxlen), th->n_rnn_seg), dim3(256), 0, st, P, G, th->d_seg_off,
                       th->d_seg_len, th->pnorms, (float)th->opts.regularization_weight);
  }
  seg_norms(th, G, th->gnorms);
  th->adam_step += 1;
  const double bc1 = 1.0 - std::pow(0.9, (double)th->adam_step);
  const double bc2 = 1.0 - std::pow(0.999, (double)th->adam_step);
  AdamConsts ac{(float)(th->opts.learning_rate / bc1), (float)std::sqrt(bc2), (float)th->opts.grad_max_norm,
                th->n_rnn_seg, th->n_rnn, th->n_adam, th->s2(), (int64_t)D};
  hipLaunchKernelGGL(k_clip_adam, dim3(grid1(th->n_total)), dim3(256), 0, st, ac, th->gnorms, P, G, th->Mo, th->Vo);
  TCHK(hipGetLastError());
  th->iter += 1;
  if (out_losses) {
    TCHK(hipMemcpyAsync(out_losses, th->losses, 4 * sizeof(float), hipMemcpyDeviceToHost, st));
    TCHK(hipStreamSynchronize(st));
  }
  return UIS_OK;
}

UIS_EXPORT int32_t uis_train_param_count(uis_trainer* th, int64_t* count_out) {
  if (!th || !count_out) return tfail(UIS_ERR_INVALID_ARG, "uis_train_param_count: NULL argument");
  *count_out = th->n_total;
  return UIS_OK;
}

static int32_t copy_out(uis_trainer* th, const float* src, float* dst, int64_t count, const char* what) {
  if (!th || !dst) return tfail(UIS_ERR_INVALID_ARG, std::string(what) + ": NULL argument");
  if (count != th->n_total)
    return tfail(UIS_ERR_DIM_MISMATCH, std::string(what) + ": count must be uis_train_param_count()");
  TCHK(hipSetDevice(th->device));
  TCHK(hipMemcpyAsync(dst, src, sizeof(float) * (size_t)count, hipMemcpyDeviceToHost, th->stream));
  TCHK(hipStreamSynchronize(th->stream));
  return UIS_OK;
}

UIS_EXPORT int32_t uis_train_get_params(uis_trainer* th, float* params_out, int64_t count) {
  return copy_out(th, th ? th->P : nullptr, params_out, count, "uis_train_get_params");
}

UIS_EXPORT int32_t uis_train_get_grads(uis_trainer* th, float* grads_out, int64_t count) {
  return copy_out(th, th ? th->G : nullptr, grads_out, count, "uis_train_get_grads");
}

UIS_EXPORT void uis_train_destroy(uis_trainer* th) {
  if (!th) return;
  (void)hipSetDevice(th->device);
  if (th->stream) (void)hipStreamSynchronize(th->stream);
  free_all(th);
  delete th;
}
