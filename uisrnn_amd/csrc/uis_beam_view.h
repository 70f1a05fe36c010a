// uis_beam_view.h -- reading what a decode or a session left in an utterance's tables: ONE statement of the rule for
// the readouts and the between-launch session kernels (uis_nbest / _posterior / _commit / _retire.hip).
// backtrace_body, k_backtrace and k_backtrace_window (uis_kernels.hip) carry the older copy of the same rule; they sit
// inside the one-launch decode kernels and on the benchmark's path and are left exactly as they are.
//
// #included by uis_decoder.hip after the handle and the decode kernels (DecodeState), ahead of uis_stream.hip
// (k_stream_bindings) and uis_nbest.hip.

namespace {

// ---- a record word of DecodeState::bp: label | parent << 16.  Ranks at or above a step's beam width were never written
// (stale words, any bit pattern): the parent is clamped, so a walk stays inside the utterance's records.
__device__ __forceinline__ int rec_label(uint32_t v) { return (int)(v & 0xffffu); }
__device__ __forceinline__ int rec_parent(uint32_t v, int B) {
  const int p = (int)(v >> 16);
  return p < B ? p : B - 1;
}

// ---- what is readable of utterance u right now
struct BeamView {
  long N, T;      // frames of the readout; steps run (sessions: T = N = avail, else tau * N)
  int par;        // parity of the beam tables that hold the final beam
  int nb, live;   // beam_n clamped to [0, B]; the hypotheses a readout shows: 0 for an utterance flagged in the overflow word
  size_t e;       // first index of its rank rows in the beam tables of parity `par`
  uint32_t* bp;   // its first record
};

// A window of N == 0 frames: the readouts and the prune show nothing (nb = 0 without reading beam_n); the retire
// kernels read beam_n all the same -- a window that a commit emptied still holds its one hypothesis, an utterance
// that has received nothing the empty one.
enum EmptyWindow { EMPTY_WINDOW_SHOWS_NOTHING, EMPTY_WINDOW_KEEPS_BEAM };

// `count` names the final beam's parity: the steps T for look_ahead 1 records, the windows run for bp16 records
__device__ __forceinline__ BeamView beam_view_at(const DecodeState& st, int u, long N, long T, long count, EmptyWindow empty) {
  const int par = (int)(count & 1);
  int nb = (N > 0 || empty == EMPTY_WINDOW_KEEPS_BEAM) ? st.beam_n[(size_t)par * st.U + u] : 0;
  nb = nb < 0 ? 0 : (nb > st.B ? st.B : nb);
  return BeamView{N, T, par, nb, st.overflow[u] ? 0 : nb, ((size_t)par * st.U + u) * st.B,
                  st.bp + (size_t)st.tau * st.off[u] * st.B};
}

// k_backtrace's rule: avail for sessions, tau * N otherwise
__device__ __forceinline__ BeamView beam_view(const DecodeState& st, int u, EmptyWindow empty = EMPTY_WINDOW_SHOWS_NOTHING) {
  const long N = st.avail ? (long)st.avail[u] : (long)(st.off[u + 1] - st.off[u]);
  const long T = st.avail ? N : (long)st.tau * N;
  return beam_view_at(st, u, N, T, T, empty);
}

// ---- the last N of T steps cut into at most 64 segments, walked downwards: segment l = steps hi(l) .. lo(l),
// hi(0) = T - 1, the last lo = T - N
struct SegGeom {
  long T, N, seg;
  int nseg;
  __device__ __forceinline__ long hi(int l) const { return T - 1 - (long)l * seg; }
  __device__ __forceinline__ long lo(int l) const { return hi(l) - seg + 1 < T - N ? T - N : hi(l) - seg + 1; }
};

__device__ __forceinline__ SegGeom seg_geom(long T, long N) {
  const long seg = (N + 63) / 64;
  return SegGeom{T, N, seg, N > 0 ? (int)((N + seg - 1) / seg) : 0};
}

// one chain through segment l from entry rank r: f(step, record word), downwards
template <typename F>
__device__ __forceinline__ void walk_segment(const uint32_t* bp, int B, const SegGeom& g, int l, int r, F f) {
  const long lo = g.lo(l);
  for (long s = g.hi(l); s >= lo; --s) {
    const uint32_t v = bp[(size_t)s * B + r];
    f(s, v);
    r = rec_parent(v, B);
  }
}

// ---- the dynamic LDS of nbest_segment_maps / nbest_stitch (uis_nbest.hip): [0, 16) a word of the kernel's own;
// bt_map [64][B] exit rank by segment and entry rank; ent [B][64] entry rank by hypothesis and segment; `more`: whatever
// a kernel asked for on top (k_posterior: [B] float64, [B] float32)
__host__ __device__ inline size_t nbest_lds_bytes(int B) { return (size_t)16 + (size_t)128 * B; }
inline size_t posterior_lds_bytes(int B) { return nbest_lds_bytes(B) + (size_t)12 * B; }

struct NbestLds { int* word; unsigned char *bt_map, *ent, *more; };

__device__ __forceinline__ NbestLds nbest_lds(unsigned char* base, int B) {
  return NbestLds{reinterpret_cast<int*>(base), base + 16, base + 16 + (size_t)64 * B, base + nbest_lds_bytes(B)};
}

// ---- moving data in place inside one workgroup, where sources and destinations overlap: every thread loads its
// elements into registers, then this, then it stores.  The wait makes sure the loads have RETURNED before the barrier
// lets anyone store.  For a move towards lower addresses in ascending tiles one such barrier per tile is enough: tile
// t's destination lies below every later tile's source, and whatever it overwrites inside tile t is in registers.
__device__ __forceinline__ void loads_before_stores() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

#define UIS_COMMIT_THREADS 256
#define UIS_COMMIT_TILE_WORDS 1024  // move_words_down (k_commit_move): words per tile = one 16-byte access per thread

// one tile of K elements per thread, i0 + k * UIS_COMMIT_THREADS: those of [0, n)
template <typename T, int K>
__device__ __forceinline__ void move_tile(T* dst, const T* src, long i0, long n) {
  T v[K];
#pragma unroll
  for (int k = 0; k < K; ++k)
    if (i0 + k * UIS_COMMIT_THREADS < n) v[k] = src[i0 + k * UIS_COMMIT_THREADS];
  loads_before_stores();
#pragma unroll
  for (int k = 0; k < K; ++k)
    if (i0 + k * UIS_COMMIT_THREADS < n) dst[i0 + k * UIS_COMMIT_THREADS] = v[k];
}

// words [0, words) from src to dst < src by a whole workgroup of UIS_COMMIT_THREADS threads (all of them call): 16
// bytes per thread where both are aligned, then the scalar tail of up to three words -- above everything stored so
// far and below nothing still to be read --, else the scalar path at the same tile size
__device__ __forceinline__ void move_words_down(uint32_t* dst, const uint32_t* src, long words) {
  const long tid = threadIdx.x;
  if (((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15u) == 0) {
    const long nvec = words >> 2;
    for (long base = 0; base < nvec; base += UIS_COMMIT_TILE_WORDS / 4)
      move_tile<uint4, 1>(reinterpret_cast<uint4*>(dst), reinterpret_cast<const uint4*>(src), base + tid, nvec);
    move_tile<uint32_t, 1>(dst, src, (nvec << 2) + tid, words);
  } else {
    for (long base = 0; base < words; base += UIS_COMMIT_TILE_WORDS)
      move_tile<uint32_t, UIS_COMMIT_TILE_WORDS / UIS_COMMIT_THREADS>(dst, src, base + tid, words);
  }
}

}  // namespace
