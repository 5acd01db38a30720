// negatives.hip — srw_skipgram_batch's negatives (by vertex weight, kept out of their own window) and the two count vectors people
// weight by: srw_negative_weights_set, srw_graph_degrees_device, srw_path_vertex_counts.  Semantics: include/stellar_rw.h, DESIGN §7d.
//
//   weight table   w[nV] uint32 over V (the present vertices, ascending) -> cdf[i] = w[0] + .. + w[i] (uint64, a rocprim inclusive scan
//                  through a u32 -> u64 transform iterator), T = cdf[nV - 1] > 0, and a guide table: guide[b], b = 0 .. 2^g, is the index
//                  the draw u = b << (64 - g) selects (guide[2^g]: the index t = T - 1 selects, the largest any u can).  t = (u * T) >> 64
//                  is monotone in u, so the draw whose top g bits are b lies in [guide[b], guide[b + 1]]; 2^g is the power of two at or
//                  above nV, which makes that bracket one or two entries for an even table.
//   k_neg_draw     one lane per Philox block of one window — four uniform or two weighted negatives —, a group of G lanes per row as
//                  k_skipgram_fill has it (the same G from the same shape), reading off[r], off[r + 1] of the scan srw_skipgram_windows
//                  left on the handle.  A weighted draw is two guide words, then a binary search over the bracket whose body is selects
//                  (its trip count is the only thing that differs between lanes), then verts[] (and orig_id[] on compacted ids).  With
//                  exclusion the row is staged in LDS once (rows beyond SG_LDS_STRIDE_MAX ints are read from global memory) and a lane
//                  redraws the entries of its block that hit their window, attempt a on key word 1 + 2 a (uniform) / 2 + 2 a (weighted):
//                  one Philox block per attempt serves every entry of the block that is still open; lanes with nothing open leave the
//                  loop.
//   k_vertex_count one lane per path element, 64-bit atomics into a per-slot array (the rank array on compacted ids), equal slots of a
//                  wave added once: up to VC_ROUNDS leaders are taken out by ballot before the lanes that are left add on their own — a
//                  star graph sends half of all tokens to one counter.  k_vertex_gather then reads the slots in V order.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "engine.h"

namespace srw {
namespace {
constexpr int NG_TPB = 256;
constexpr int NG_BLOCKS_PER_CU = 8;
constexpr int64_t NG_LDS_STRIDE_MAX = 2048;  // as skipgram.hip's SG_LDS_STRIDE_MAX: the same rows are staged
constexpr int VC_ROUNDS = 4;

struct WidenU32 {
  __host__ __device__ inline uint64_t operator()(uint32_t w) const { return (uint64_t)w; }
};
using WidenIter = rocprim::transform_iterator<const uint32_t *, WidenU32, uint64_t>;

// smallest i in [lo, hi] with cdf[i] > t, given cdf[hi] > t.  The body is two selects; a bracket of length 0 does not enter it.
__device__ inline uint32_t cdf_search(const uint64_t *__restrict__ cdf, uint32_t lo, uint32_t hi, uint64_t t) {
  uint32_t len = hi - lo;                              // candidates below hi
  while (len > 0) {
    const uint32_t half = len >> 1;
    const bool right = cdf[lo + half] <= t;
    lo = right ? lo + half + 1 : lo;
    len = right ? len - half - 1 : half;
  }
  return lo;
}

// guide[b] for b = 0 .. 2^g: one lane per entry, a search over the whole table (once per srw_negative_weights_set)
__global__ __launch_bounds__(NG_TPB) void k_neg_guide(const uint64_t *__restrict__ cdf, uint32_t nV, uint64_t T, int32_t g,
                                                      uint32_t *__restrict__ guide) {
  const uint64_t b = (uint64_t)blockIdx.x * NG_TPB + threadIdx.x, nb = (uint64_t)1 << g;
  if (b > nb) return;
  const uint64_t t = b == nb ? T - 1 : (g ? __umul64hi(b << (64 - g), T) : 0);   // (g == 0: b == 0, u == 0)
  guide[b] = cdf_search(cdf, 0u, nV - 1, t);           // (cdf[nV - 1] == T > t)
}

struct DrawArgs {
  const int32_t *paths;   // [n][stride] (read with exclusion only)
  const int64_t *off;     // [n + 1]
  int64_t n, stride;
  int32_t C, K, KB;       // KB: Philox blocks per window = ceil(K / 4) uniform, ceil(K / 2) weighted
  uint32_t seed, epoch;
  int32_t *neg;
  const int32_t *verts;   // present vertices, ascending (ids, or slots when orig_id != nullptr)
  uint32_t nV;
  const int32_t *orig_id;
  int32_t vmin;
  const uint64_t *cdf;    // the table in force (weighted form only)
  const uint32_t *guide;
  uint64_t T;
  int32_t gbits;
  int32_t draws;          // attempts per entry: max_draws with exclusion, else 1
  int32_t neg_vec;        // a lane's block is one aligned vector store (16 bytes uniform, 8 bytes weighted)
};

// EXCL: 0 no exclusion, 1 the row staged in LDS, 2 the row read from global memory
template <int G, bool WEIGHTED, int EXCL>
__global__ __launch_bounds__(NG_TPB) void k_neg_draw(const DrawArgs a) {
  extern __shared__ int32_t s_rows[];
  constexpr int GPB = NG_TPB / G;
  constexpr int E = WEIGHTED ? 2 : 4;                  // negatives per Philox block
  const int gl = (int)threadIdx.x & (G - 1);
  const int grp = (int)threadIdx.x / G;
  const int32_t *row = s_rows + (EXCL == 1 ? (int64_t)grp * a.stride : 0);
  const int32_t C = a.C, K = a.K, KB = a.KB;
  const int32_t nj0 = gl / KB, nb0 = gl % KB, uj = G / KB, ub = G % KB;   // the lane's first block as (j, b) and its step: the only divisions

  for (int64_t r = (int64_t)blockIdx.x * GPB + grp; r < a.n; r += (int64_t)gridDim.x * GPB) {
    const int64_t o = a.off[r];
    const int32_t cnt = (int32_t)(a.off[r + 1] - o);
    if (cnt <= 0) continue;
    if constexpr (EXCL == 1) {
      const int32_t len = cnt + C - 1;                 // (<= stride: WindowCount)
      const int32_t *__restrict__ src = a.paths + r * a.stride;
      int32_t *wrow = s_rows + (int64_t)grp * a.stride;
      for (int32_t k = gl; k < len; k += G) wrow[k] = src[k];
      __builtin_amdgcn_wave_barrier();                 // (the group is part of one wave: LDS serves its writes and reads in order)
    }
    if constexpr (EXCL == 2) row = a.paths + r * a.stride;

    int32_t *__restrict__ nd = a.neg + o * K;
    const int64_t units = (int64_t)cnt * KB;
    int32_t nj = nj0, nb = nb0;
    for (int64_t u = gl; u < units; u += G) {
      const int32_t k0 = E * nb;
      int32_t x[E];
      uint32_t open = 0;                               // entries of this block that have no accepted draw yet
#pragma unroll
      for (int e = 0; e < E; ++e) { x[e] = 0; open |= (k0 + e < K) ? 1u << e : 0u; }
      for (int32_t at = 0; open; ++at) {
        uint32_t w[4];
        philox4x32_10((uint32_t)r, (uint32_t)nj, (uint32_t)nb, a.epoch, a.seed, (WEIGHTED ? 2u : 1u) + 2u * (uint32_t)at, w);
        const bool last = at + 1 >= a.draws;
#pragma unroll
        for (int e = 0; e < E; ++e) {
          if (!(open >> e & 1u)) continue;
          uint32_t i;
          if constexpr (WEIGHTED) {
            const uint64_t uu = ((uint64_t)w[2 * e] << 32) | w[2 * e + 1];
            const uint64_t t = __umul64hi(uu, a.T);
            const uint64_t b = a.gbits ? uu >> (64 - a.gbits) : 0;
            i = cdf_search(a.cdf, a.guide[b], a.guide[b + 1], t);
          } else {
            i = __umulhi(w[e], a.nV);
          }
          int32_t v = a.verts[i];
          if (a.orig_id) v = a.orig_id[v - a.vmin];
          bool hit = false;
          if constexpr (EXCL != 0) {
            if (!last)
              for (int32_t c = 0; c < C; ++c) hit |= row[nj + c] == v;     // (nj + C - 1 <= cnt + C - 2: inside the row)
          }
          x[e] = v;
          open &= hit ? ~0u : ~(1u << e);
        }
      }
      int32_t *d = nd + (int64_t)nj * K + k0;
      if constexpr (WEIGHTED) {
        if (a.neg_vec) *reinterpret_cast<int2 *>(d) = make_int2(x[0], x[1]);
        else {
          d[0] = x[0];                                 // (k0 < K: nb < KB)
          if (k0 + 1 < K) d[1] = x[1];
        }
      } else {
        if (a.neg_vec) *reinterpret_cast<int4 *>(d) = make_int4(x[0], x[1], x[2], x[3]);
        else {
          d[0] = x[0];
          if (k0 + 1 < K) d[1] = x[1];
          if (k0 + 2 < K) d[2] = x[2];
          if (k0 + 3 < K) d[3] = x[3];
        }
      }
      nj += uj; nb += ub;
      if (nb >= KB) { nb -= KB; ++nj; }
    }
    if constexpr (EXCL == 1) __builtin_amdgcn_wave_barrier();   // the row's reads are issued before the next row is staged over it
  }
}

template <int G, bool WEIGHTED, int EXCL>
void launch_draw(srw_handle *h, const DrawArgs &a) {
  constexpr int GPB = NG_TPB / G;
  const int64_t want = (a.n + GPB - 1) / GPB;
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)h->n_cus * NG_BLOCKS_PER_CU));
  const size_t lds = EXCL == 1 ? (size_t)GPB * (size_t)a.stride * 4 : 0;
  hipLaunchKernelGGL((k_neg_draw<G, WEIGHTED, EXCL>), dim3(blocks), dim3(NG_TPB), lds, h->stream, a);
  SRW_HIP(hipGetLastError());
}

template <bool WEIGHTED, int EXCL>
void launch_draw_g(srw_handle *h, const DrawArgs &a, int G) {
  if (G == 4) launch_draw<4, WEIGHTED, EXCL>(h, a);
  else if (G == 16) launch_draw<16, WEIGHTED, EXCL>(h, a);
  else launch_draw<64, WEIGHTED, EXCL>(h, a);
}

// ---- counts ----
// slots[n_slots + 1] (zeroed by the caller): occurrences per slot; slots[n_slots]: ids that are no vertex of the graph
__global__ __launch_bounds__(NG_TPB) void k_vertex_count(const int32_t *__restrict__ paths, const int32_t *__restrict__ lens, int64_t n,
                                                         int64_t stride, const Row *__restrict__ rows, const int32_t *__restrict__ orig_id,
                                                         int64_t n_slots, int32_t vmin, unsigned long long *__restrict__ slots) {
  const int64_t step = (int64_t)gridDim.x * NG_TPB, first = (int64_t)blockIdx.x * NG_TPB + threadIdx.x;
  int64_t r = first / stride, c = first % stride;      // the lane's first element as (row, column) and its step: the only divisions
  const int64_t dr = step / stride, dc = step % stride;
  const int lane = (int)threadIdx.x & 63;
  // (every lane of a wave takes the same number of turns or one fewer; a lane past the end stays in the loop as idle, so that the
  // ballots below always see whole waves)
  const int64_t total = n * stride;
  for (int64_t t0 = first - lane; t0 < total; t0 += step) {
    const bool in = t0 + lane < total;
    int64_t s = -1;                                    // the element's slot; -1: no element here; n_slots: no vertex of the graph
    if (in) {
      const int32_t l = lens[r] < stride ? lens[r] : (int32_t)stride;
      if (c < l) {
        s = vertex_slot(paths[r * stride + c], rows, orig_id, n_slots, vmin);   // (device_common.h: k_sgns_step resolves the same way)
      }
    }
    // equal slots of the wave are added once: up to VC_ROUNDS leaders, then every lane that is left for itself
    bool todo = s >= 0;
    for (int round = 0; round < VC_ROUNDS; ++round) {
      const unsigned long long left = __ballot(todo);
      if (!left) break;
      const int lead = __ffsll((long long)left) - 1;
      const int64_t ls = ((int64_t)__shfl((int)(s >> 32), lead) << 32) | (uint32_t)__shfl((int)(uint32_t)s, lead);
      const bool same = todo && s == ls;
      const unsigned long long m = __ballot(same);
      if (lane == lead) atomicAdd(&slots[ls], (unsigned long long)__popcll(m));
      todo = todo && !same;
    }
    if (todo) atomicAdd(&slots[s], 1ull);
    r += dr; c += dc;
    if (c >= stride) { c -= stride; ++r; }
  }
}

__global__ __launch_bounds__(NG_TPB) void k_vertex_gather(const unsigned long long *__restrict__ slots, const int32_t *__restrict__ verts,
                                                          int64_t nV, int32_t vmin, int64_t *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * NG_TPB + threadIdx.x;
  if (i < nV) out[i] = (int64_t)slots[(int64_t)verts[i] - vmin];
}

__global__ __launch_bounds__(NG_TPB) void k_degree_gather(const Row *__restrict__ rows, const int32_t *__restrict__ verts, int64_t nV,
                                                          int32_t vmin, int64_t *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * NG_TPB + threadIdx.x;
  if (i < nV) out[i] = (int64_t)rows[(int64_t)verts[i] - vmin].deg;
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + NG_TPB - 1) / NG_TPB); }
}  // namespace

void negative_weights_set(srw_handle *h, const uint32_t *d_w, int64_t n) {
  Graph &g = h->g;
  hipStream_t st = h->stream;
  const uint32_t nV = (uint32_t)n;
  // into buffers of its own: the table in force stays as it is until T > 0 is known
  DevBuf<uint64_t> cdf; DevBuf<uint32_t> guide;
  cdf.alloc((size_t)n);
  const WidenIter in(d_w, WidenU32());
  size_t tb = 0;
  SRW_HIP(rocprim::inclusive_scan(nullptr, tb, in, cdf.p, (size_t)n, rocprim::plus<uint64_t>(), st));
  h->sg_temp.ensure(std::max<size_t>(tb, 1));
  SRW_HIP(rocprim::inclusive_scan((void *)h->sg_temp.p, tb, in, cdf.p, (size_t)n, rocprim::plus<uint64_t>(), st));
  uint64_t T = 0;
  SRW_HIP(hipMemcpyAsync(&T, cdf.p + (n - 1), 8, hipMemcpyDeviceToHost, st));
  SRW_HIP(hipStreamSynchronize(st));
  if (T == 0) throw Error(SRW_ERR_INVALID, "srw_negative_weights_set: every weight is 0 (the table in force is unchanged)");
  int32_t gb = 0;
  while (((int64_t)1 << gb) < n) ++gb;                 // 2^g >= nV (nV < 2^31: g <= 31)
  const int64_t entries = ((int64_t)1 << gb) + 1;
  guide.alloc((size_t)entries);
  hipLaunchKernelGGL(k_neg_guide, dim3(blocks_for(entries)), dim3(NG_TPB), 0, st, (const uint64_t *)cdf.p, nV, T, gb, guide.p);
  SRW_HIP(hipGetLastError());
  SRW_HIP(hipStreamSynchronize(st));
  g.neg_cdf = std::move(cdf); g.neg_guide = std::move(guide);
  g.neg_total = T; g.neg_gbits = gb; g.has_neg = true;
}

void negative_weights_clear(srw_handle *h) {
  h->g.neg_cdf.release(); h->g.neg_guide.release();
  h->g.neg_total = 0; h->g.neg_gbits = 0; h->g.has_neg = false;
}

void graph_degrees_device(srw_handle *h, int64_t *d_out) {
  const Graph &g = h->g;
  if (g.n_vertices <= 0) return;
  hipLaunchKernelGGL(k_degree_gather, dim3(blocks_for(g.n_vertices)), dim3(NG_TPB), 0, h->stream, (const Row *)g.rows.p,
                     (const int32_t *)g.verts.p, g.n_vertices, g.vmin, d_out);
  SRW_HIP(hipGetLastError());
  SRW_HIP(hipStreamSynchronize(h->stream));
}

int64_t path_vertex_counts(srw_handle *h, const int32_t *d_paths, const int32_t *d_lens, int64_t n, int64_t stride, int64_t *d_counts) {
  const Graph &g = h->g;
  hipStream_t st = h->stream;
  h->vc_slots.ensure((size_t)g.n_slots + 1);
  SRW_HIP(hipMemsetAsync(h->vc_slots.p, 0, ((size_t)g.n_slots + 1) * 8, st));
  if (n > 0) {
    const int64_t want = (n * stride + NG_TPB - 1) / NG_TPB;
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)h->n_cus * NG_BLOCKS_PER_CU));
    hipLaunchKernelGGL(k_vertex_count, dim3(blocks), dim3(NG_TPB), 0, st, d_paths, d_lens, n, stride, (const Row *)g.rows.p,
                       g.compact ? (const int32_t *)g.orig_id.p : nullptr, g.n_slots, g.vmin, h->vc_slots.p);
    SRW_HIP(hipGetLastError());
  }
  if (g.n_vertices > 0) {
    hipLaunchKernelGGL(k_vertex_gather, dim3(blocks_for(g.n_vertices)), dim3(NG_TPB), 0, st, (const unsigned long long *)h->vc_slots.p,
                       (const int32_t *)g.verts.p, g.n_vertices, g.vmin, d_counts);
    SRW_HIP(hipGetLastError());
  }
  unsigned long long unknown = 0;
  SRW_HIP(hipMemcpyAsync(&unknown, h->vc_slots.p + g.n_slots, 8, hipMemcpyDeviceToHost, st));
  SRW_HIP(hipStreamSynchronize(st));
  return (int64_t)unknown;
}

int64_t skipgram_batch(srw_handle *h, const int32_t *d_paths, const int32_t *d_lens, int64_t n, int64_t stride,
                       const srw_skipgram_batch_params &bp, int32_t *d_pos, int32_t *d_neg, int64_t cap_windows) {
  if (n == 0) return 0;
  const int32_t C = bp.context, K = bp.num_negatives;
  // windows, off[] and pos: srw_skipgram_windows' scan and its fill kernel, asked for no negatives
  const srw_skipgram_params sp{C, 0, bp.seed, bp.epoch};
  const int64_t W = skipgram_windows(h, d_paths, d_lens, n, stride, sp, d_pos, nullptr, cap_windows);
  if (!d_pos || W > cap_windows || W == 0 || K == 0) return W;
  const Graph &g = h->g;
  if (g.n_vertices <= 0) throw Error(SRW_ERR_INVALID, "srw_skipgram_batch: the loaded graph has no vertex to draw negatives from");

  const bool weighted = g.has_neg, excl = bp.exclude_window != 0;
  DrawArgs a{};
  a.paths = d_paths; a.off = h->sg_off.p; a.n = n; a.stride = stride;
  a.C = C; a.K = K; a.KB = weighted ? (K + 1) / 2 : (K + 3) / 4;
  a.seed = bp.seed; a.epoch = bp.epoch;
  a.neg = d_neg;
  a.verts = g.verts.p; a.nV = (uint32_t)g.n_vertices;
  a.orig_id = g.compact ? g.orig_id.p : nullptr; a.vmin = g.vmin;
  a.cdf = weighted ? g.neg_cdf.p : nullptr; a.guide = weighted ? g.neg_guide.p : nullptr;
  a.T = g.neg_total; a.gbits = g.neg_gbits;
  a.draws = excl ? bp.max_draws : 1;
  a.neg_vec = weighted ? (K % 2 == 0 && ((uintptr_t)d_neg & 7u) == 0) : (K % 4 == 0 && ((uintptr_t)d_neg & 15u) == 0);
  // lanes per row: k_skipgram_fill's rule, from the output of a full row
  const int64_t full = (stride - C + 1) * (int64_t)C;
  const bool staged = stride <= NG_LDS_STRIDE_MAX;
  const int G = !staged ? 64 : full <= 16 ? 4 : full <= 128 ? 16 : 64;
  if (!excl) { if (weighted) launch_draw_g<true, 0>(h, a, G); else launch_draw_g<false, 0>(h, a, G); }
  else if (staged) { if (weighted) launch_draw_g<true, 1>(h, a, G); else launch_draw_g<false, 1>(h, a, G); }
  else { if (weighted) launch_draw<64, true, 2>(h, a); else launch_draw<64, false, 2>(h, a); }
  SRW_HIP(hipStreamSynchronize(h->stream));
  return W;
}

}  // namespace srw
