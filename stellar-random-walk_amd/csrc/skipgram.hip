// skipgram.hip — srw_skipgram_windows: the batch a skip-gram / node2vec negative-sampling loss consumes, built from paths that are
// already in HBM (the last walk's result, or a caller's arrays in the same layout).
//
//   pos [W][C]  every run of C consecutive vertices of every path, row-major then window start ascending: row r owns the contiguous
//               stretch pos[off[r] * C .. (off[r] + cnt[r]) * C), cnt[r] = max(0, lens[r] - C + 1), off = exclusive prefix sum of cnt;
//               element t of that stretch is paths[r][t / C + t % C].  No window holds a -1: the tail of a dead-ended row has none.
//   neg [W][K]  K vertices per window, uniform over the present vertices V (ascending, what srw_graph_vertices lists):
//               word = philox4x32_10(ctr = (r, j, k >> 2, epoch), key = (seed, 1))[k & 3],  neg = V[(word * nV) >> 32]
//               — keyed by (row within the call, window start, k), never by the window's place in the output, and on a stream
//               of its own (the walk's key is (seed, 0)).  Not filtered against the window's own vertices.
//
// Two steps on the handle's stream:
//   1. off[n + 1]: rocprim::exclusive_scan over a transform iterator that turns lens[r] into cnt[r] (no cnt array); off[n] = W is
//      the call's only read-back.  The count-only form is a rocprim::reduce over the same iterator.
//   2. k_skipgram_fill: a group of G lanes per row (G = 64: one wave per row; 16 or 4 when a whole row's output is a few dozen
//      ints, so that short rows do not leave most of a wave idle), grid-stride over rows.  The row goes into LDS once (one coalesced
//      read), then the lanes walk the row's output stretch in 16-byte vectors: the stretch is cut at the 16-byte boundaries of the
//      destination, whole vectors are one dwordx4 store, the first and the last one go element by element.  (j, c) = (t / C, t % C)
//      is never divided out per element: a lane divides once per launch (its first vector) and steps by the constant
//      (4 G / C, 4 G % C) per pass and by one inside a vector.  The negatives follow in the same kernel — off and cnt are at hand,
//      and the Philox arithmetic (ten rounds per four words) overlaps the store stream: a lane computes one Philox block =
//      the four negatives k = 4 b .. 4 b + 3 of one (r, j, b) and stores them as one vector when K % 4 == 0 and neg is aligned.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "engine.h"

namespace srw {
namespace {
constexpr int SG_TPB = 256;
constexpr int SG_BLOCKS_PER_CU = 8;
constexpr int64_t SG_LDS_STRIDE_MAX = 2048;   // rows up to this many ints are staged in LDS (G = 64: 4 rows x 8 KiB per block at most)

// cnt[r] from lens[r]; index n (one past the rows) counts 0, so that the exclusive scan over n + 1 entries leaves W in off[n].
// A length above the stride (never written by srw_walk) is read as the stride: the fill kernel then stays inside the row.
struct WindowCount {
  const int32_t *lens;
  int64_t n;
  int32_t stride, C;
  __host__ __device__ inline int64_t operator()(int64_t r) const {
    if (r >= n) return 0;
    const int32_t l = lens[r] < stride ? lens[r] : stride;
    return l >= C ? (int64_t)(l - C + 1) : (int64_t)0;
  }
};
using CountIter = rocprim::transform_iterator<rocprim::counting_iterator<int64_t>, WindowCount, int64_t>;

struct FillArgs {
  const int32_t *paths;   // [n][stride]
  const int64_t *off;     // [n + 1]
  int64_t n, stride;
  int32_t C, K, KB;       // KB = ceil(K / 4): Philox blocks per window
  uint32_t seed, epoch;
  int32_t *pos, *neg;
  const int32_t *verts;   // present vertices, ascending (ids, or slots when orig_id != nullptr)
  uint32_t nV;
  const int32_t *orig_id;
  int32_t vmin;
  int32_t neg_vec;        // K % 4 == 0 and neg 16-byte aligned: a Philox block is one 16-byte store
};

template <int G, bool STAGE>
__global__ __launch_bounds__(SG_TPB) void k_skipgram_fill(const FillArgs a) {
  extern __shared__ int32_t s_rows[];
  constexpr int GPB = SG_TPB / G;                      // rows in flight per block
  const int gl = (int)threadIdx.x & (G - 1);
  const int grp = (int)threadIdx.x / G;
  int32_t *row = s_rows + (STAGE ? (int64_t)grp * a.stride : 0);
  const int32_t C = a.C, K = a.K, KB = a.KB;
  // the lane's first element 4 * gl of a stretch as (j, c), its step per pass, and the same for its Philox blocks: the only divisions
  const int32_t j0 = (4 * gl) / C, c0 = (4 * gl) % C, dj = (4 * G) / C, dc = (4 * G) % C;
  const int32_t nj0 = K ? gl / KB : 0, nb0 = K ? gl % KB : 0, uj = K ? G / KB : 0, ub = K ? G % KB : 0;

  for (int64_t r = (int64_t)blockIdx.x * GPB + grp; r < a.n; r += (int64_t)gridDim.x * GPB) {
    const int64_t o = a.off[r];
    const int32_t cnt = (int32_t)(a.off[r + 1] - o);
    if (cnt <= 0) continue;
    const int32_t len = cnt + C - 1;                   // (<= stride: WindowCount)
    const int32_t *__restrict__ src = a.paths + r * a.stride;
    if constexpr (STAGE) {
      for (int32_t k = gl; k < len; k += G) row[k] = src[k];
      __builtin_amdgcn_wave_barrier();                 // (the group is part of one wave: LDS serves its writes and reads in order)
    }
    auto at = [&](int32_t i) -> int32_t {
      i = min(max(i, 0), len - 1);                     // (elements outside the stretch are computed and not stored)
      if constexpr (STAGE) return row[i]; else return src[i];
    };

    // ---- pos: the stretch [0, cnt * C) at dst, walked from the 16-byte boundary at or below dst (element -al)
    int32_t *__restrict__ dst = a.pos + o * C;
    const int32_t al = (int32_t)(((uintptr_t)dst >> 2) & 3u);
    const int64_t total = (int64_t)cnt * C;
    int32_t j = j0, c = c0 - al;
    while (c < 0) { c += C; --j; }                     // (at most three turns)
    for (int64_t t = 4 * gl - al; t < total; t += 4 * G) {
      int4 v;
      int32_t i = j + c, cc = c;
      v.x = at(i); i = cc + 1 < C ? i + 1 : i + 2 - C; cc = cc + 1 < C ? cc + 1 : 0;
      v.y = at(i); i = cc + 1 < C ? i + 1 : i + 2 - C; cc = cc + 1 < C ? cc + 1 : 0;
      v.z = at(i); i = cc + 1 < C ? i + 1 : i + 2 - C;
      v.w = at(i);
      if (t >= 0 && t + 3 < total) *reinterpret_cast<int4 *>(dst + t) = v;
      else {                                           // the first and the last vector of a stretch
        if (t >= 0) dst[t] = v.x;
        if (t + 1 >= 0 && t + 1 < total) dst[t + 1] = v.y;
        if (t + 2 >= 0 && t + 2 < total) dst[t + 2] = v.z;
        if (t + 3 < total) dst[t + 3] = v.w;           // (t + 3 >= 0 always: t >= -3)
      }
      j += dj; c += dc;
      if (c >= C) { c -= C; ++j; }
    }

    // ---- neg: Philox block u = j * KB + b of the row -> neg[(o + j) * K + 4 b ..]
    if (K > 0) {
      int32_t *__restrict__ nd = a.neg + o * K;
      const int64_t units = (int64_t)cnt * KB;
      int32_t nj = nj0, nb = nb0;
      for (int64_t u = gl; u < units; u += G) {
        uint32_t w[4];
        philox4x32_10((uint32_t)r, (uint32_t)nj, (uint32_t)nb, a.epoch, a.seed, 1u, w);
        int4 v;
        int32_t x[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          x[e] = a.verts[__umulhi(w[e], a.nV)];
          if (a.orig_id) x[e] = a.orig_id[x[e] - a.vmin];
        }
        v.x = x[0]; v.y = x[1]; v.z = x[2]; v.w = x[3];
        int32_t *d = nd + (int64_t)nj * K + 4 * nb;
        if (a.neg_vec) *reinterpret_cast<int4 *>(d) = v;
        else {
          const int32_t k = 4 * nb;
          d[0] = v.x;                                  // (k < K: nb < KB)
          if (k + 1 < K) d[1] = v.y;
          if (k + 2 < K) d[2] = v.z;
          if (k + 3 < K) d[3] = v.w;
        }
        nj += uj; nb += ub;
        if (nb >= KB) { nb -= KB; ++nj; }
      }
    }
    if constexpr (STAGE) __builtin_amdgcn_wave_barrier();   // the row's reads are issued before the next row is staged over it
  }
}

template <int G, bool STAGE>
void launch_fill(srw_handle *h, const FillArgs &a) {
  constexpr int GPB = SG_TPB / G;
  const int64_t want = (a.n + GPB - 1) / GPB;
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)h->n_cus * SG_BLOCKS_PER_CU));
  const size_t lds = STAGE ? (size_t)GPB * (size_t)a.stride * 4 : 0;
  hipLaunchKernelGGL((k_skipgram_fill<G, STAGE>), dim3(blocks), dim3(SG_TPB), lds, h->stream, a);
  SRW_HIP(hipGetLastError());
}
}  // namespace

int64_t skipgram_windows(srw_handle *h, const int32_t *d_paths, const int32_t *d_lens, int64_t n, int64_t stride,
                         const srw_skipgram_params &sp, int32_t *d_pos, int32_t *d_neg, int64_t cap_windows) {
  if (n == 0) return 0;
  hipStream_t st = h->stream;
  const int32_t C = sp.context, K = sp.num_negatives;
  const WindowCount count{d_lens, n, (int32_t)stride, C};
  const CountIter in(rocprim::counting_iterator<int64_t>(0), count);
  int64_t W = 0;

  if (!d_pos) {                                        // count only: one reduction, its result in the last 8 bytes of the temporary storage
    size_t tb = 0;
    SRW_HIP(rocprim::reduce(nullptr, tb, in, (int64_t *)nullptr, (int64_t)0, (size_t)n, rocprim::plus<int64_t>(), st));
    tb = (tb + 7) & ~(size_t)7;
    h->sg_temp.ensure(tb + 8);
    int64_t *d_w = reinterpret_cast<int64_t *>(h->sg_temp.p + tb);
    SRW_HIP(rocprim::reduce((void *)h->sg_temp.p, tb, in, d_w, (int64_t)0, (size_t)n, rocprim::plus<int64_t>(), st));
    SRW_HIP(hipMemcpyAsync(&W, d_w, 8, hipMemcpyDeviceToHost, st));
    SRW_HIP(hipStreamSynchronize(st));
    return W;
  }

  h->sg_off.ensure((size_t)n + 1);
  size_t tb = 0;
  SRW_HIP(rocprim::exclusive_scan(nullptr, tb, in, h->sg_off.p, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), st));
  h->sg_temp.ensure(std::max<size_t>(tb, 1));       // (never a null pointer: that would ask rocprim for the size again)
  SRW_HIP(rocprim::exclusive_scan((void *)h->sg_temp.p, tb, in, h->sg_off.p, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), st));
  SRW_HIP(hipMemcpyAsync(&W, h->sg_off.p + n, 8, hipMemcpyDeviceToHost, st));
  SRW_HIP(hipStreamSynchronize(st));
  if (W > cap_windows || W == 0) return W;             // (the caller turns W > cap_windows into the error; nothing is written)
  if (K > 0 && h->g.n_vertices <= 0) throw Error(SRW_ERR_INVALID, "srw_skipgram_windows: the loaded graph has no vertex to draw negatives from");

  FillArgs a{};
  a.paths = d_paths; a.off = h->sg_off.p; a.n = n; a.stride = stride;
  a.C = C; a.K = K; a.KB = (K + 3) / 4;
  a.seed = sp.seed; a.epoch = sp.epoch;
  a.pos = d_pos; a.neg = d_neg;
  a.verts = h->g.verts.p; a.nV = (uint32_t)h->g.n_vertices;
  a.orig_id = h->g.compact ? h->g.orig_id.p : nullptr; a.vmin = h->g.vmin;
  a.neg_vec = (K > 0 && K % 4 == 0 && ((uintptr_t)d_neg & 15u) == 0) ? 1 : 0;
  // lanes per row from the output of a full row, (stride - C + 1) * C ints (>= stride): up to 16 -> 4 lanes, up to 128 -> 16, else a wave
  const int64_t full = (stride - C + 1) * (int64_t)C;
  if (stride > SG_LDS_STRIDE_MAX) launch_fill<64, false>(h, a);
  else if (full <= 16) launch_fill<4, true>(h, a);
  else if (full <= 128) launch_fill<16, true>(h, a);
  else launch_fill<64, true>(h, a);
  SRW_HIP(hipStreamSynchronize(st));
  return W;
}

}  // namespace srw
