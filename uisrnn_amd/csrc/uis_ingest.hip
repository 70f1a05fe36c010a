// uis_ingest.hip -- device tensors in: k_ingest gathers row blocks that already live in HBM (float32, float64, float16
// or bfloat16, any row stride) into the packed float32 [F, D] stream every decode path starts from (included by
// uis_decoder.hip).
//
//   ingest_validate()  the host-side checks of a uis_tensor list (before any GPU work) and its row count
//   ingest_enqueue()   the descriptor table (one H2D), the wait for the producer's stream, ONE launch of k_ingest
//                      (a push sends the table inside its own staging block: ingest_fill_table + ingest_launch)
//
// Arithmetic.  float64 -> float32 is the hardware convert (v_cvt_f32_f64): round to nearest even under the library's
// denormal mode (float32 subnormals kept), which is what the host cast team of uis_decode_f64 and numpy's
// astype(float32) produce -- subnormal results and overflow to +-inf included (tests/test_gpu_ingest.py decides).
// float16 -> float32 (v_cvt_f32_f16) is exact, subnormal inputs included; bfloat16 -> float32 is the 16-bit shift.
//
// Work.  The packed stream is cut into items of 8 consecutive floats of one row (the last item of a row is short where D
// is no multiple of 8); thread t of the launch owns items t, so every output element has exactly one writer and no
// atomics are needed.  An item finds its block by a binary search of its row in the blocks' first rows: the table the
// host sends is one 32-byte record per BLOCK, not per workgroup, so a one-frame push of 64 slots uploads 2 KB whatever D
// is and a 64 x 500 decode the same 2 KB.  Empty blocks share their successor's first row and the search (the LAST block
// whose first row is <= the row) passes over them.
//
// Memory.  Where the host found a block's base and row pitch to be multiples of 16 bytes, D a multiple of 4 and the
// output base 16-byte aligned (IngestBlock::vec), full groups of four elements travel as 16-byte loads (two per group
// for float64, one per EIGHT elements for the 16-bit types, 8 bytes for a 16-bit group of four at a row's end) and
// 16-byte stores.  Everything else -- an odd base, a pitch that misaligns every other row, D % 4 != 0, a row's tail --
// goes element by element.
#ifndef UIS_INGEST_HIP_
#define UIS_INGEST_HIP_

#define UIS_INGEST_THREADS 256
#define UIS_INGEST_ITEMS 2  // items per thread: a workgroup takes 512 items = 4096 floats of the stream at D % 8 == 0

struct IngestBlock {
  const void* data;
  long long row0;        // the block's first row in the packed stream
  long long row_stride;  // elements between two rows
  int32_t dtype;         // UIS_DTYPE_*
  int32_t vec;           // 1: 16-byte accesses are aligned for every row of this block
};
static_assert(sizeof(IngestBlock) == 32, "one descriptor is two 16-byte words");

__device__ __forceinline__ float ingest_f16(unsigned short bits) {
  _Float16 v;
  __builtin_memcpy(&v, &bits, 2);
  return (float)v;  // (v_cvt_f32_f16)
}
__device__ __forceinline__ float ingest_bf16(unsigned short bits) { return __uint_as_float((unsigned)bits << 16); }
__device__ __forceinline__ float ingest_16(unsigned short bits, bool bf) { return bf ? ingest_bf16(bits) : ingest_f16(bits); }

__device__ __forceinline__ float ingest_elem(const char* row, int c, int dtype) {
  switch (dtype) {
    case UIS_DTYPE_F32: return reinterpret_cast<const float*>(row)[c];
    case UIS_DTYPE_F64: return (float)reinterpret_cast<const double*>(row)[c];
    case UIS_DTYPE_F16: return ingest_f16(reinterpret_cast<const unsigned short*>(row)[c]);
    default: return ingest_bf16(reinterpret_cast<const unsigned short*>(row)[c]);
  }
}

__device__ __forceinline__ f32x4 ingest_quad16(unsigned lo, unsigned hi, bool bf) {
  f32x4 v;
  v[0] = ingest_16((unsigned short)(lo & 0xffffu), bf); v[1] = ingest_16((unsigned short)(lo >> 16), bf);
  v[2] = ingest_16((unsigned short)(hi & 0xffffu), bf); v[3] = ingest_16((unsigned short)(hi >> 16), bf);
  return v;
}

// tab[n]: the blocks in stream order; F = rows of the stream; opr = ceil(D / 8) items per row
__global__ __launch_bounds__(UIS_INGEST_THREADS) void k_ingest(const IngestBlock* __restrict__ tab, int n, long long F, int D,
                                                                int opr, float* __restrict__ out) {
  const long long total = F * opr;
  for (int k = 0; k < UIS_INGEST_ITEMS; ++k) {
    const long long item = ((long long)blockIdx.x * UIS_INGEST_ITEMS + k) * UIS_INGEST_THREADS + threadIdx.x;
    if (item >= total) return;
    const long long row = item / opr;
    const int c0 = (int)(item - row * opr) * 8;
    int lo = 0, hi = n - 1;  // (tab[0].row0 == 0 <= row < F: the block found holds the row)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (tab[mid].row0 <= row) lo = mid; else hi = mid - 1;
    }
    const IngestBlock b = tab[lo];
    const int esz = b.dtype == UIS_DTYPE_F64 ? 8 : b.dtype == UIS_DTYPE_F32 ? 4 : 2;
    const char* src = static_cast<const char*>(b.data) + (size_t)((row - b.row0) * b.row_stride) * esz;
    float* dst = out + (size_t)row * D;
    const bool bf = b.dtype == UIS_DTYPE_BF16;
    if (b.vec && esz == 2 && c0 + 8 <= D) {  // eight 16-bit elements: one 16-byte load, two 16-byte stores
      const uint4 w = *reinterpret_cast<const uint4*>(src + (size_t)c0 * 2);
      *reinterpret_cast<f32x4*>(dst + c0) = ingest_quad16(w.x, w.y, bf);
      *reinterpret_cast<f32x4*>(dst + c0 + 4) = ingest_quad16(w.z, w.w, bf);
      continue;
    }
    for (int c = c0; c < c0 + 8 && c < D; c += 4) {
      if (b.vec && c + 4 <= D) {
        f32x4 v;
        if (esz == 4) {
          v = *reinterpret_cast<const f32x4*>(src + (size_t)c * 4);
        } else if (esz == 8) {
          const double2 a = *reinterpret_cast<const double2*>(src + (size_t)c * 8);
          const double2 d = *reinterpret_cast<const double2*>(src + (size_t)c * 8 + 16);
          v[0] = (float)a.x; v[1] = (float)a.y; v[2] = (float)d.x; v[3] = (float)d.y;
        } else {
          const uint2 w = *reinterpret_cast<const uint2*>(src + (size_t)c * 2);
          v = ingest_quad16(w.x, w.y, bf);
        }
        *reinterpret_cast<f32x4*>(dst + c) = v;
      } else {
        for (int j = c; j < c + 4 && j < D; ++j) dst[j] = ingest_elem(src, j, b.dtype);
      }
    }
  }
}

namespace {

inline int ingest_elem_bytes(int32_t dtype) {
  return dtype == UIS_DTYPE_F64 ? 8 : dtype == UIS_DTYPE_F32 ? 4 : (dtype == UIS_DTYPE_F16 || dtype == UIS_DTYPE_BF16) ? 2 : 0;
}

// The checks of a uis_tensor list, on the host, before any GPU work; *rows_out = the rows of the packed stream.
int ingest_validate(const char* who, const uis_tensor* blocks, int32_t n, int D, int64_t* rows_out) {
  const char* const w = who;
  if (n < 0 || (n > 0 && !blocks)) return fail(UIS_ERR_INVALID_ARG, std::string(w) + ": null tensor list or negative count");
  int64_t F = 0;
  for (int i = 0; i < n; ++i) {
    const uis_tensor& t = blocks[i];
    const auto at = [&] { return std::string(w) + ": tensor " + std::to_string(i); };  // (the text of a refusal only)
    const int esz = ingest_elem_bytes(t.dtype);
    if (!esz) return fail(UIS_ERR_INVALID_ARG, at() + " has an unknown dtype (UIS_DTYPE_F32 / _F64 / _F16 / _BF16)");
    if (t.rows < 0) return fail(UIS_ERR_INVALID_ARG, at() + " has a negative row count");
    if (t.rows == 0) continue;
    if (!t.data) return fail(UIS_ERR_INVALID_ARG, at() + " has rows but no data");
    if (t.row_stride < D) return fail(UIS_ERR_INVALID_ARG, at() + ": row_stride is below observation_dim (rows would overlap)");
    if (reinterpret_cast<uintptr_t>(t.data) % (uintptr_t)esz) return fail(UIS_ERR_INVALID_ARG, at() + ": data is not aligned to its element size");
    F += t.rows;
    if (F > 0x7fffffff00LL) return fail(UIS_ERR_UNSUPPORTED, std::string(w) + ": too many rows");
  }
  *rows_out = F;
  return UIS_OK;
}

// Whether every row of the block may be read, and its part of the stream written, 16 bytes at a time.
inline bool ingest_vec_ok(const uis_tensor& t, int D, const float* d_out) {
  const uintptr_t esz = (uintptr_t)ingest_elem_bytes(t.dtype);
  return D % 4 == 0 && reinterpret_cast<uintptr_t>(d_out) % 16 == 0 && reinterpret_cast<uintptr_t>(t.data) % 16 == 0 &&
         ((uintptr_t)t.row_stride * esz) % 16 == 0;
}

// The kernel's table of a validated list whose stream goes to d_out, into `tab` (host memory the caller uploads).
void ingest_fill_table(IngestBlock* tab, const uis_tensor* blocks, int32_t n, int D, const float* d_out) {
  int64_t row0 = 0;
  for (int i = 0; i < n; ++i) {
    const uis_tensor& t = blocks[i];
    tab[i] = IngestBlock{t.rows ? t.data : nullptr, (long long)row0, (long long)t.row_stride, t.dtype,
                         t.rows && ingest_vec_ok(t, D, d_out) ? 1 : 0};
    row0 += t.rows;
  }
}

// The table d_tab (already on its way to the device on the handle's stream) -> d_out [F, D] on the handle's stream,
// behind everything `producer_stream` holds at this moment.  Nothing is waited for here: the caller's next work on the
// handle's stream is ordered behind the launch.
int ingest_launch(uis_handle* h, const IngestBlock* d_tab, int32_t n, int64_t F, void* producer_stream, float* d_out) {
  const int D = h->m.D;
  // the tensors were written on the producer's stream (NULL: the default stream), which this library's own
  // non-blocking stream does not follow by itself
  if (!h->ev_producer) HIPCHK(hipEventCreateWithFlags(&h->ev_producer, hipEventDisableTiming));
  HIPCHK(hipEventRecord(h->ev_producer, static_cast<hipStream_t>(producer_stream)));
  HIPCHK(hipStreamWaitEvent(h->stream, h->ev_producer, 0));
  const int opr = (D + 7) / 8;
  const long long per_wg = (long long)UIS_INGEST_THREADS * UIS_INGEST_ITEMS;
  const long long wgs = ((long long)F * opr + per_wg - 1) / per_wg;
  if (wgs > 0x7fffffffLL) return fail(UIS_ERR_UNSUPPORTED, "too many rows for one ingest launch");
  hipLaunchKernelGGL(k_ingest, dim3((unsigned)wgs), dim3(UIS_INGEST_THREADS), 0, h->stream, d_tab, (int)n, (long long)F, D, opr, d_out);
  HIPCHK(hipGetLastError());
  return UIS_OK;
}

// The validated list -> d_out: the table through the handle's own pinned block and device copy (one H2D), the launch.
int ingest_enqueue(uis_handle* h, const uis_tensor* blocks, int32_t n, int64_t F, void* producer_stream, float* d_out,
                   const UisPoison& poison) {
  if (F == 0) return UIS_OK;
  const size_t bytes = (size_t)n * sizeof(IngestBlock);
  if (bytes > h->h_ingest.cap) {
    const hipError_t e = h->h_ingest.ensure(bytes + bytes / 4 + 1024, hipHostMallocDefault);
    if (e != hipSuccess) return fail(UIS_ERR_OOM, std::string("hipHostMalloc (ingest table): ") + hipGetErrorString(e));
  }
  if (int rc = h->ingest_tab.ensure(bytes)) return rc;
  poison.host(h->h_ingest.p, h->h_ingest.cap);
  HIPCHK(poison.device(h->ingest_tab.p, h->ingest_tab.cap, h->stream));
  ingest_fill_table(h->h_ingest.as<IngestBlock>(), blocks, n, h->m.D, d_out);
  HIPCHK(hipMemcpyAsync(h->ingest_tab.p, h->h_ingest.p, bytes, hipMemcpyHostToDevice, h->stream));
  return ingest_launch(h, h->ingest_tab.as<IngestBlock>(), n, F, producer_stream, d_out);
}

}  // namespace

#endif  // UIS_INGEST_HIP_
