// topk.hip — srw_topk_rows: the k best rows of a float32 table [n_rows][D] for every query, by cosine or dot product, without ever
// forming the Q x n_rows product; srw_vertex_rows: vertex ids -> positions in V.  Semantics: include/stellar_rw.h, DESIGN §7f.
//
// Queries go in passes of QB (32 up to D = 256, 16 up to 512, 8 beyond: the staged queries stay within 32 KiB of LDS).  Per pass:
//   k_topk_prep   one wave per query: the query's row index is range-checked BEFORE it is multiplied into an address, the vector (a
//                 table row or the caller's) is copied to qstage [QB][D], its sum of squares is taken by one lane in the order
//                 d = 0, 1, ... and excl[q] becomes the excluded row, -1 (none) or -2 (the query is skipped).
//   k_topk_scan   a persistent grid of 128-thread blocks over tiles of 128 rows, ONE ROW PER LANE.  The queries sit in LDS for the
//                 whole pass.  A tile comes in chunks of 32 dimensions: 128 x 32 floats, fetched with plain dword loads (a row of a
//                 table that is only 4-byte aligned earns nothing wider) into registers one chunk ahead, stored to a padded LDS
//                 image [128][33] and read back row-wise, conflict-free.  Lane = row reads its 32 values once and feeds QB
//                 accumulators with fmaf; the query operand is a wave-uniform 16-byte LDS read (a broadcast) per four FMAs.  dot and
//                 the row's sum of squares are fmaf chains over d = 0, 1, ..., D - 1 (then zeros up to the chunk's end, which change
//                 no value): the score of (query, row) depends on those two vectors alone.
//                 Every wave keeps, per query, a sorted list of 64 keys, entry j in lane j (two registers per query), and compares
//                 its 64 fresh keys with the list's k-th key: one ballot per (tile, query).  Only where a lane beats it does the slow
//                 path run: per such lane one readlane, one ballot for the position, one lane shift.  The lists are flushed to
//                 lists [n_waves][QB][k] at the end.
//   k_topk_merge  one wave per query: the n_waves * k keys through the same list, then rows and scores are written.
// A key is (order-preserving image of the score) << 32 | (0xFFFFFFFF - row): the larger key is the better row, ties need no case of
// their own, and 0 — below every key a row can have — is padding.  No float atomics, no order that depends on timing.
#include "engine.h"
#include "wave_primitives.h"

namespace srw {
namespace {
constexpr int TK_TPB = 128;             // rows per tile, one per lane
constexpr int TK_DC = 32;               // dimensions per chunk
constexpr int TK_LD = TK_DC + 1;        // the LDS image's row stride: lane l reads bank (l + d) % 32
constexpr int TK_BLOCKS_PER_CU = 3;          // 3 x (32 KiB of queries + 16.5 KiB of image) of the CU's 160 KiB
constexpr int32_t TK_SKIP = -2;

__device__ inline uint64_t readlane_u64(uint64_t v, int lane) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
  return ((uint64_t)hi << 32) | lo;
}

// NaN ranks as -inf, -0 as +0; then the integer order of the image is the float order
__device__ inline uint64_t topk_key(float score, uint32_t row) {
  uint32_t b = __float_as_uint(score);
  if ((b & 0x7FFFFFFFu) > 0x7F800000u) b = 0xFF800000u;
  if ((b << 1) == 0u) b = 0u;
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((uint64_t)b << 32) | (uint64_t)(0xFFFFFFFFu - row);
}
__device__ inline float topk_key_score(uint64_t key) {
  const uint32_t b = (uint32_t)(key >> 32);
  return __uint_as_float((b & 0x80000000u) ? (b & 0x7FFFFFFFu) : ~b);
}

// list: 64 keys in descending order, entry j in lane j; cand: one key per lane (0: none).  Afterwards entries 0 .. k - 1 are the k
// largest of what they were and the candidates.  Keys of rows are distinct, so no comparison below meets a tie other than 0 == 0.
__device__ inline void topk_offer(uint64_t &list, uint64_t cand, int k, int lane) {
  uint64_t thr = readlane_u64(list, k - 1);
  unsigned long long m = __ballot(cand > thr);
  while (m) {
    const int s = __ffsll(m) - 1;
    m &= m - 1;
    const uint64_t x = readlane_u64(cand, s);
    if (x > thr) {                                     // (wave-uniform)
      const int pos = __popcll(__ballot(list > x));    // <= k - 1: x beats entry k - 1
      const uint64_t up = __shfl_up((unsigned long long)list, 1);
      list = lane < pos ? list : (lane == pos ? x : up);
      thr = readlane_u64(list, k - 1);
    }
  }
}

__global__ __launch_bounds__(64) void k_topk_prep(const float *__restrict__ table, int64_t n_rows, int32_t D, const float *__restrict__ qvec,
                                                  const int32_t *__restrict__ qrow, int64_t q0, float *__restrict__ qstage,
                                                  float *__restrict__ qq, int32_t *__restrict__ excl) {
  const int lane = lane_id();
  const int64_t q = blockIdx.x, gq = q0 + q;
  const int32_t xr = qrow ? qrow[gq] : -1;
  const bool in_range = (uint32_t)xr < (uint32_t)n_rows;            // (n_rows < 2^31; -1 is not in range)
  const bool skip = qvec ? (xr != -1 && !in_range) : !in_range;
  const float *src = qvec ? qvec + gq * D : table + (in_range ? (int64_t)xr : 0) * D;      // no xr reaches an address unchecked
  for (int32_t d = lane; d < D; d += 64) qstage[q * D + d] = skip ? 0.0f : src[d];
  if (lane == 0) {
    float s = 0.0f;
    if (!skip) for (int32_t d = 0; d < D; ++d) { const float v = src[d]; s = fmaf(v, v, s); }
    qq[q] = s;
    excl[q] = skip ? TK_SKIP : (in_range ? xr : -1);
  }
}

struct ScanArgs {
  const float *table; int64_t n_rows; int32_t D, Dp, k, metric, nq;
  const float *qstage, *qq; const int32_t *excl;
  unsigned long long *lists;            // [n_waves][QB][k]
};

template <int QB>
__global__ __launch_bounds__(TK_TPB, 2) void k_topk_scan(const ScanArgs a) {
  extern __shared__ float4 tk_smem[];
  float *sq = reinterpret_cast<float *>(tk_smem);      // [QB][Dp], zero beyond D and beyond nq
  float *st = sq + (size_t)QB * a.Dp;                  // [128][TK_LD]
  const int tid = (int)threadIdx.x, lane = lane_id();
  const int32_t D = a.D, Dp = a.Dp, k = a.k, nq = a.nq;
  for (int32_t i = tid; i < QB * Dp; i += TK_TPB) {
    const int32_t q = i / Dp, d = i - q * Dp;
    sq[i] = (q < nq && d < D) ? a.qstage[(int64_t)q * D + d] : 0.0f;
  }
  uint64_t list[QB];
#pragma unroll
  for (int q = 0; q < QB; ++q) list[q] = 0;
  const int64_t n_tiles = (a.n_rows + TK_TPB - 1) / TK_TPB;
  const int32_t n_chunks = Dp / TK_DC;
  // element i of a thread's share of a chunk: row (i * 128 + tid) / 32 of the tile, dimension (i * 128 + tid) % 32 of the chunk
  const int ld_row = tid >> 5, ld_d = tid & 31;
  float pre[TK_DC];
  auto fetch = [&](int64_t tile, int32_t c) {
    const int32_t d = c * TK_DC + ld_d;
#pragma unroll
    for (int i = 0; i < TK_DC; ++i) {
      const int64_t row = tile * TK_TPB + i * 4 + ld_row;
      pre[i] = (row < a.n_rows && d < D) ? a.table[row * D + d] : 0.0f;
    }
  };
  int64_t tile = blockIdx.x;
  if (tile < n_tiles) fetch(tile, 0);
  for (; tile < n_tiles; tile += gridDim.x) {
    float acc[QB], rr = 0.0f;
#pragma unroll
    for (int q = 0; q < QB; ++q) acc[q] = 0.0f;
    for (int32_t c = 0; c < n_chunks; ++c) {
      __syncthreads();                                 // the image's last readers are done (and, first time round, sq is written)
#pragma unroll
      for (int i = 0; i < TK_DC; ++i) st[(i * 4 + ld_row) * TK_LD + ld_d] = pre[i];
      __syncthreads();
      if (c + 1 < n_chunks) fetch(tile, c + 1);
      else if (tile + gridDim.x < n_tiles) fetch(tile + gridDim.x, 0);
      const float *mine = st + tid * TK_LD;
      const float *qc = sq + c * TK_DC;
#pragma unroll 1
      for (int d4 = 0; d4 < TK_DC; d4 += 4) {
        const float r0 = mine[d4], r1 = mine[d4 + 1], r2 = mine[d4 + 2], r3 = mine[d4 + 3];
        rr = fmaf(r0, r0, rr); rr = fmaf(r1, r1, rr); rr = fmaf(r2, r2, rr); rr = fmaf(r3, r3, rr);
#pragma unroll
        for (int q = 0; q < QB; ++q) {
          const float4 qv = *reinterpret_cast<const float4 *>(qc + (size_t)q * Dp + d4);
          acc[q] = fmaf(qv.x, r0, acc[q]); acc[q] = fmaf(qv.y, r1, acc[q]);
          acc[q] = fmaf(qv.z, r2, acc[q]); acc[q] = fmaf(qv.w, r3, acc[q]);
        }
      }
    }
    const int64_t row = tile * TK_TPB + tid;
    const float rnorm = sqrtf(rr);
#pragma unroll
    for (int q = 0; q < QB; ++q) {
      if (q < nq) {                                    // (wave-uniform)
        const int32_t ex = a.excl[q];
        float s = acc[q];
        if (a.metric == 0) {
          const float qs = a.qq[q];
          s = (qs == 0.0f || rr == 0.0f) ? 0.0f : s / (sqrtf(qs) * rnorm);
        }
        const uint64_t cand = (row < a.n_rows && ex != TK_SKIP && row != (int64_t)ex) ? topk_key(s, (uint32_t)row) : 0;
        topk_offer(list[q], cand, k, lane);
      }
    }
  }
  const int64_t wave = (int64_t)blockIdx.x * (TK_TPB / 64) + (tid >> 6);
#pragma unroll
  for (int q = 0; q < QB; ++q)
    if (lane < k) a.lists[(wave * QB + q) * k + lane] = list[q];
}

__global__ __launch_bounds__(64) void k_topk_merge(const unsigned long long *__restrict__ lists, int64_t n_waves, int32_t QB, int32_t k,
                                                   const int32_t *__restrict__ excl, int64_t q0, int32_t *__restrict__ rows,
                                                   float *__restrict__ scores, unsigned long long *__restrict__ skipped) {
  const int lane = lane_id();
  const int64_t q = blockIdx.x;
  uint64_t list = 0;
  if (excl[q] == TK_SKIP) {
    if (lane == 0) atomicAdd(skipped, 1ull);
  } else {
    const int64_t total = n_waves * k;
    for (int64_t base = 0; base < total; base += 64) {
      const int64_t i = base + lane;
      uint64_t cand = 0;
      if (i < total) { const int64_t w = i / k; cand = lists[(w * QB + q) * k + (i - w * k)]; }
      topk_offer(list, cand, k, lane);
    }
  }
  if (lane < k) {
    const int64_t o = (q0 + q) * k + lane;
    rows[o] = list ? (int32_t)(0xFFFFFFFFu - (uint32_t)list) : -1;
    scores[o] = list ? topk_key_score(list) : -__builtin_inff();
  }
}

template <int QB>
void launch_scan(srw_handle *h, const ScanArgs &a, unsigned blocks) {
  const size_t lds = ((size_t)QB * a.Dp + (size_t)TK_TPB * TK_LD) * sizeof(float);
  hipLaunchKernelGGL(k_topk_scan<QB>, dim3(blocks), dim3(TK_TPB), lds, h->stream, a);
  SRW_HIP(hipGetLastError());
}

__global__ __launch_bounds__(256) void k_vertex_rows(const int32_t *__restrict__ ids, int64_t n, const Row *__restrict__ rows,
                                                     const int32_t *__restrict__ orig_id, const int32_t *__restrict__ vpos, int64_t n_slots,
                                                     int32_t vmin, int32_t *__restrict__ out, unsigned long long *__restrict__ unknown) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t s = vertex_slot(ids[i], rows, orig_id, n_slots, vmin);
  const int32_t p = s < n_slots ? vpos[s] : -1;
  out[i] = p;
  if (p < 0) atomicAdd(unknown, 1ull);
}
}  // namespace

int64_t topk_rows(srw_handle *h, const float *d_table, int64_t n_rows, const float *d_qvec, const int32_t *d_qrow, int64_t n_queries,
                  const srw_topk_params &tp, int32_t *d_rows, float *d_scores) {
  hipStream_t st = h->stream;
  const int32_t D = tp.dim, k = tp.k;
  const int32_t QB = D <= 256 ? 32 : D <= 512 ? 16 : 8;
  const int32_t Dp = (D + TK_DC - 1) / TK_DC * TK_DC;
  const int64_t n_tiles = (n_rows + TK_TPB - 1) / TK_TPB;
  const unsigned blocks = (unsigned)std::min<int64_t>(n_tiles, (int64_t)h->n_cus * TK_BLOCKS_PER_CU);
  const int64_t n_waves = (int64_t)blocks * (TK_TPB / 64);
  // scratch of one pass, whatever n_queries is: the lists, then the staged queries, their sums of squares, excl, the skip count
  const size_t lists_b = (size_t)std::max<int64_t>(n_waves, 1) * QB * k * 8, stage_b = (size_t)QB * D * 4, qq_b = (size_t)QB * 4;
  h->topk_scratch.ensure(lists_b + stage_b + 2 * qq_b + 8);
  char *base = h->topk_scratch.p;
  unsigned long long *lists = (unsigned long long *)base;
  float *qstage = (float *)(base + lists_b);
  float *qq = (float *)(base + lists_b + stage_b);
  int32_t *excl = (int32_t *)(base + lists_b + stage_b + qq_b);
  unsigned long long *skipped = (unsigned long long *)(base + lists_b + stage_b + 2 * qq_b);
  SRW_HIP(hipMemsetAsync(skipped, 0, 8, st));
  for (int64_t q0 = 0; q0 < n_queries; q0 += QB) {
    const int32_t nq = (int32_t)std::min<int64_t>(QB, n_queries - q0);
    hipLaunchKernelGGL(k_topk_prep, dim3((unsigned)nq), dim3(64), 0, st, d_table, n_rows, D, d_qvec, d_qrow, q0, qstage, qq, excl);
    SRW_HIP(hipGetLastError());
    if (blocks) {
      ScanArgs a{d_table, n_rows, D, Dp, k, tp.metric, nq, qstage, qq, excl, lists};
      switch (QB) {
        case 32: launch_scan<32>(h, a, blocks); break;
        case 16: launch_scan<16>(h, a, blocks); break;
        default: launch_scan<8>(h, a, blocks); break;
      }
    }
    hipLaunchKernelGGL(k_topk_merge, dim3((unsigned)nq), dim3(64), 0, st, lists, n_waves, QB, k, excl, q0, d_rows, d_scores, skipped);
    SRW_HIP(hipGetLastError());
  }
  unsigned long long n_skip = 0;
  SRW_HIP(hipMemcpyAsync(&n_skip, skipped, 8, hipMemcpyDeviceToHost, st));
  SRW_HIP(hipStreamSynchronize(st));
  return (int64_t)n_skip;
}

int64_t vertex_rows(srw_handle *h, const int32_t *d_ids, int64_t n, int32_t *d_rows) {
  const Graph &g = h->g;
  hipStream_t st = h->stream;
  ensure_vpos(h);
  h->sgns_skipped.ensure(1);
  SRW_HIP(hipMemsetAsync(h->sgns_skipped.p, 0, 8, st));
  hipLaunchKernelGGL(k_vertex_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_ids, n, (const Row *)g.rows.p,
                     g.compact ? (const int32_t *)g.orig_id.p : nullptr, (const int32_t *)g.vpos.p, g.n_slots, g.vmin, d_rows,
                     h->sgns_skipped.p);
  SRW_HIP(hipGetLastError());
  unsigned long long unknown = 0;
  SRW_HIP(hipMemcpyAsync(&unknown, h->sgns_skipped.p, 8, hipMemcpyDeviceToHost, st));
  SRW_HIP(hipStreamSynchronize(st));
  return (int64_t)unknown;
}

}  // namespace srw
