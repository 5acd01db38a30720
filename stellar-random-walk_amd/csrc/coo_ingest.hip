// coo_ingest.hip — the front door of srw_load_coo_device: edge arrays that are already in HBM (a training loop's edge_index).
//
// The builders behind every load (compact_ids, build_graph_from_device_lines, build_graph_blocked) take device arrays of int32 ids
// and the id range [vmin, vmax].  What a caller's tensors lack is that range, the check that an int64 id fits the engine's int32
// ids, and — for int64 — the narrowed arrays.  k_coo_ingest streams both id columns ONCE and produces all three: 8 (int32) or
// 16 + 8 (int64: read + narrowed write) bytes per line, against the 16 bytes per line the host entry point moves over PCIe after a
// single-threaded scan.  It is bound by HBM bandwidth: 16-byte loads, one per lane and pass, a grid sized from the CU count.
//
// Reductions: per lane over the grid-stride loop, per wave (DPP / shuffles), per block through LDS, then one atomicMin / atomicMax
// per block on three words in HBM, which the host reads back in one 16-byte copy — the call's only read-back unless an id does not
// fit (then 8 more bytes: the id itself, for the message).
#include <cstring>

#include "engine.h"
#include "wave_primitives.h"

namespace srw {
namespace {
// The launch geometry (tests/test_gpu_load_device.py reads these three lines to place its edge counts around one pass of the grid):
// blockIdx.y selects the column (src / dst), and every lane takes one 16-byte vector per pass of the grid-stride loop.
constexpr int INGEST_TPB = 256;
constexpr int INGEST_BLOCKS_PER_CU = 4;
constexpr int INGEST_VEC_BYTES = 16;

constexpr unsigned long long NO_BAD = ~0ull;

struct IngestWords {        // the three words of the reduction, as the host initialises and reads them
  int32_t lo, hi;           // smallest / largest id of both columns (int64: of the narrowed ids)
  unsigned long long bad;   // smallest (line << 1 | column) of an int64 id outside int32; all ones: none
};

template <typename T> struct IdVec;
template <> struct IdVec<int32_t> { using type = int4; };
template <> struct IdVec<int64_t> { using type = longlong2; };

__device__ inline unsigned long long wave_min_u64(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) { const unsigned long long x = __shfl_xor(v, o); v = x < v ? x : v; }
  return v;
}

// src / dst: n ids each, naturally aligned.  A column is cut into a head (the ids in front of its first 16-byte boundary), a body of
// whole 16-byte vectors and a tail; head and tail (fewer than a vector each) go element by element.  int64: out_src / out_dst receive
// the ids narrowed to int32 — the host offsets each so that out + head is 8-byte aligned, and a body vector is stored as one int2.
template <typename T>
__global__ __launch_bounds__(INGEST_TPB) void k_coo_ingest(const T *__restrict__ src, const T *__restrict__ dst, int64_t n,
                                                           int32_t *__restrict__ out_src, int32_t *__restrict__ out_dst, IngestWords *words) {
  using Vec = typename IdVec<T>::type;
  constexpr int V = INGEST_VEC_BYTES / (int)sizeof(T);
  constexpr bool WIDE = sizeof(T) == 8;
  const unsigned long long col = blockIdx.y;
  const T *__restrict__ in = col ? dst : src;
  int32_t *__restrict__ out = col ? out_dst : out_src;
  const int64_t head = min(n, (int64_t)(((INGEST_VEC_BYTES - ((uintptr_t)in & (INGEST_VEC_BYTES - 1))) & (INGEST_VEC_BYTES - 1)) / sizeof(T)));
  const int64_t n_vec = (n - head) / V;
  const int64_t tail0 = head + n_vec * V;
  const int64_t t = blockIdx.x * (int64_t)INGEST_TPB + threadIdx.x, stride = (int64_t)gridDim.x * INGEST_TPB;

  int32_t lo = 2147483647, hi = -2147483647 - 1;
  unsigned long long bad = NO_BAD;
  auto fold = [&](int64_t i, T v) -> int32_t {
    const int32_t x = (int32_t)v;
    lo = min(lo, x); hi = max(hi, x);
    if constexpr (WIDE) {
      const unsigned long long word = ((unsigned long long)i << 1) | col;
      bad = ((int64_t)x != (int64_t)v && word < bad) ? word : bad;
    }
    return x;
  };

  const Vec *__restrict__ vin = reinterpret_cast<const Vec *>(in + head);
  for (int64_t k = t; k < n_vec; k += stride) {
    const Vec v = vin[k];
    const int64_t i = head + k * V;
    if constexpr (WIDE) {
      int2 o;
      o.x = fold(i, v.x); o.y = fold(i + 1, v.y);
      *reinterpret_cast<int2 *>(out + i) = o;
    } else {
      fold(i, v.x); fold(i + 1, v.y); fold(i + 2, v.z); fold(i + 3, v.w);
    }
  }
  for (int64_t i = t; i < head; i += stride) {                    // (fewer than V ids: the first lanes of the first block)
    const int32_t x = fold(i, in[i]);
    if constexpr (WIDE) out[i] = x;
  }
  for (int64_t i = tail0 + t; i < n; i += stride) {
    const int32_t x = fold(i, in[i]);
    if constexpr (WIDE) out[i] = x;
  }

  // wave, then block, then one atomic per word and block
  __shared__ int32_t s_lo[INGEST_TPB / 64], s_hi[INGEST_TPB / 64];
  __shared__ unsigned long long s_bad[INGEST_TPB / 64];
  lo = wave_min_i32(lo); hi = wave_max_i32(hi);
  if constexpr (WIDE) bad = wave_min_u64(bad);
  const int w = (int)(threadIdx.x >> 6);
  if (lane_id() == 0) { s_lo[w] = lo; s_hi[w] = hi; if constexpr (WIDE) s_bad[w] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < INGEST_TPB / 64; ++k) {
      lo = min(lo, s_lo[k]); hi = max(hi, s_hi[k]);
      if constexpr (WIDE) bad = s_bad[k] < bad ? s_bad[k] : bad;
    }
    if (lo <= hi) { atomicMin(&words->lo, lo); atomicMax(&words->hi, hi); }     // (a block that saw no id has nothing to say)
    if constexpr (WIDE) { if (bad != NO_BAD) atomicMin(&words->bad, bad); }
  }
}
}  // namespace

void coo_ingest(srw_handle *h, const void *d_src, const void *d_dst, int64_t n, int32_t id_type, CooIngest &out) {
  const bool wide = id_type == SRW_IDS_I64;
  const size_t elem = wide ? 8 : 4;
  if (((uintptr_t)d_src | (uintptr_t)d_dst) & (elem - 1))
    throw Error(SRW_ERR_INVALID, "srw_load_coo_device: src / dst are not aligned to their element type");
  hipStream_t st = h->stream;
  DevBuf<IngestWords> words;
  words.alloc(1);
  const IngestWords init = {2147483647, -2147483647 - 1, NO_BAD};
  SRW_HIP(hipMemcpyAsync(words.p, &init, sizeof init, hipMemcpyHostToDevice, st));
  const dim3 grid((unsigned)(h->n_cus * INGEST_BLOCKS_PER_CU), 2u);
  if (wide) {
    // out + head 8-byte aligned for the int2 stores: head is 0 or 1 ids, the narrowed column starts at the same parity
    const int pad_s = (int)(((uintptr_t)d_src >> 3) & 1u), pad_d = (int)(((uintptr_t)d_dst >> 3) & 1u);
    out.narrow_src.alloc((size_t)n + 1); out.narrow_dst.alloc((size_t)n + 1);
    int32_t *ns = out.narrow_src.p + pad_s, *nd = out.narrow_dst.p + pad_d;
    hipLaunchKernelGGL(k_coo_ingest<int64_t>, grid, dim3(INGEST_TPB), 0, st, (const int64_t *)d_src, (const int64_t *)d_dst, n, ns, nd, words.p);
    out.src = ns; out.dst = nd;
  } else {
    hipLaunchKernelGGL(k_coo_ingest<int32_t>, grid, dim3(INGEST_TPB), 0, st, (const int32_t *)d_src, (const int32_t *)d_dst, n,
                       (int32_t *)nullptr, (int32_t *)nullptr, words.p);
    out.src = (const int32_t *)d_src; out.dst = (const int32_t *)d_dst;
  }
  SRW_HIP(hipGetLastError());
  IngestWords got;
  SRW_HIP(hipMemcpyAsync(&got, words.p, sizeof got, hipMemcpyDeviceToHost, st));
  SRW_HIP(hipStreamSynchronize(st));
  if (got.bad != NO_BAD) {
    const int64_t line = (int64_t)(got.bad >> 1);
    const bool is_dst = (got.bad & 1ull) != 0;
    long long id = 0;
    SRW_HIP(hipMemcpyAsync(&id, (const int64_t *)(is_dst ? d_dst : d_src) + line, 8, hipMemcpyDeviceToHost, st));
    SRW_HIP(hipStreamSynchronize(st));
    throw Error(SRW_ERR_INVALID, std::string("srw_load_coo_device: ") + (is_dst ? "dst" : "src") + " id " + std::to_string(id) + " at line " +
                                     std::to_string(line) + " is outside int32 [-2147483648, 2147483647]");
  }
  out.vmin = got.lo; out.vmax = got.hi;
}

}  // namespace srw
