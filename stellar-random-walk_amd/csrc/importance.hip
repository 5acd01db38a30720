// importance.hip — importance neighbours of a mini-batch of seeds (gfx950): srw_importance_neighbors (include/stellar_rw.h).
// PinSAGE's neighbourhood: the T vertices that R short first-order walks with restart from a seed visit most often, with the visit
// counts.  No reference counterpart: the reference only walks.  The weighted draw is RandomSample.sample
// (M/algorithm/RandomSample.scala:12-25) through the tables a p = q = 1 walk builds; nothing else is built or kept.
//
// Two kernels per chunk of seeds, both on the handle's stream; the scratch between them is a buffer of the handle, at most
// IMP_SCRATCH_BYTES: visits [seeds of the chunk][R * L] uint32.
//
//   k_imp_walk<NT, COMPACT>   one walk (b, w) per lane, grid-stride over the 64-bit walk index; the lanes do not depend on each other and
//                             nothing is staged: no LDS.  Only the seed goes through vertex_slot; the step is k_nbr_replace's three arms
//                             (cfo_pick over the 16-byte lattice records on regular rows, fo_pick over the 32-byte records otherwise,
//                             lane_pick_sequential on ROW_IRREGULAR rows), and the picked record's link is the next row's descriptor, as
//                             in k_walk_first_order: a step is one dependent 16-byte read, no row lookup.  Visit s of walk w of seed b
//                             goes to visits[b][s * R + w] (the lanes of a wave write consecutive words) as the vertex' SLOT (engine id
//                             - vmin: unsigned, and the order of slots is the order of the input's signed ids); IMP_NONE, above every
//                             slot, stands in a place the walk never reached and for a dropped visit of the seed itself.
//   k_imp_topk<N>             one wave (a block of 64) per seed, grid-stride; N, the power of two >= R * L (64 .. 4096), is the room in
//                             LDS (16 KB).  The row is loaded compacted — the words that are not IMP_NONE, by ballot and popcount: a
//                             walk with restart leaves most of its L places empty —, padded with IMP_NONE to n, the power of two >= their
//                             number, and sorted ascending by a bitonic network (n / 2 compare-exchanges per stage, 64 per instruction,
//                             four in flight per lane); then one pass of 64 positions at a time finds the run tails (a[i] != a[i + 1]) by
//                             ballot: a tail's count is its distance to the previous tail — the highest set bit below its lane, or the
//                             last tail of the passes before, a wave-uniform carry — and goes to a 16-bit array beside the row (8 KB).
//                             Selection: every lane keeps the best of the positions it owns (i = lane + 64 t: largest count, then the
//                             smallest t, which is the smallest slot), T times the wave takes the maximum of (count << 32 | ~slot) by
//                             butterfly, lane t keeps the winner for the store, and only the winning lane looks for its next best.  The
//                             total is the number of words that were not IMP_NONE.  Slots leave as the input's ids (orig_id).
//                             N = 64 (R * L <= 64: DGL's 10 x 2) needs no LDS: one visit per lane, the network by shuffles, the tails
//                             by one more, and a lane's only position is its best.  No global atomic touches the result.
// Grid of the walk: at most IMP_BLOCKS_PER_CU blocks of 256 per CU, §7h's reasoning (16 waves per CU: ~260 000 independent request chains
// in flight); more walks than that take further trips of the grid-stride loop.  Grid of the selection: as many one-wave blocks per CU as
// their 6 N bytes of LDS admit (6 at N = 4096, the 32 waves of a CU from N = 512 down), fewer seeds than that: one block each.
#include <algorithm>
#include <string>

#include "engine.h"
#include "sampling.h"
#include "walk_shared.h"

namespace srw {
namespace {

constexpr int IMP_BLOCKS_PER_CU = 4;
constexpr int IMP_LDS_PER_CU = 160 * 1024;              // k_imp_topk<N> holds 6 N bytes per one-wave block; at most 32 waves per CU
constexpr uint32_t IMP_KEY = 65u;                      // Philox key word 1 of this stream (0 .. 32: the walk and the negatives, 64: neighbour sampling)
constexpr uint32_t IMP_NONE = 0xFFFFFFFFu;             // no visit: above every slot
constexpr size_t IMP_SCRATCH_BYTES = (size_t)1 << 30;  // the visits of one chunk of seeds
constexpr int IMP_MAX_VISITS = 4096;                   // R * L at most: what one wave sorts in LDS

__device__ inline Row imp_link_row(uint64_t link) {
  Row r;
  r.off = (int64_t)(link & CFO_NOFF_MASK); r.deg = (int32_t)((link >> 40) & 0x7FFFFFu);
  r.flags = (link >> 63) ? ROW_IRREGULAR : 0u;
  return r;
}

template <bool NT, bool COMPACT>
__global__ __launch_bounds__(TPB) void k_imp_walk(GraphView g, const int32_t *__restrict__ seeds, uint32_t *__restrict__ visits,
                                                  int64_t n_walks, int32_t R, int32_t L, uint32_t base, uint32_t seed, uint32_t epoch,
                                                  uint32_t restart_m, int32_t keep_seed, unsigned long long *unknown) {
  Bias nobias; nobias.second_order = false; nobias.need_member = false; nobias.p = nobias.q = 1.0f;
  nobias.prev = 0; nobias.prev_sids = nullptr; nobias.prev_deg = 0; nobias.vmin = g.vmin;
  const int64_t RL = (int64_t)R * L;
  for (int64_t idx = blockIdx.x * (int64_t)TPB + threadIdx.x; idx < n_walks; idx += (int64_t)gridDim.x * TPB) {
    const int64_t b = idx / R;                           // the seed's index within the chunk (seeds and base are the chunk's)
    const uint32_t w = (uint32_t)(idx - b * R);
    const int32_t sid = seeds[b];
    Row r; r.off = 0; r.deg = 0; r.flags = 0;
    uint32_t seed_slot = IMP_NONE;
    if (sid != -1) {                                     // the only id a tensor supplies: nothing is read before vertex_slot has checked it
      const int64_t s = vertex_slot(sid, g.rows, g.orig_id, g.n_slots, g.vmin);
      if (s < g.n_slots) { r = g.rows[s]; seed_slot = (uint32_t)s; }
    }
    if (unknown && seed_slot == IMP_NONE && w == 0u) atomicAdd(unknown, 1ull);
    if (keep_seed) seed_slot = IMP_NONE;                 // nothing to drop
    uint32_t *out = visits + b * RL + w;                 // visit s: out[s * R]
    const uint32_t cb = base + (uint32_t)b;
    int32_t s = 0;
    for (; s < L; ++s) {
      uint32_t o[4];
      philox4x32_10(cb, w, (uint32_t)s, epoch, seed, IMP_KEY, o);
      if (s >= 1 && (o[1] >> 8) < restart_m) break;      // restart: the walk ends (never before its first step)
      if (r.deg == 0) break;                             // a dead end, or no vertex at all
      const uint32_t m = o[0] >> 8;
      int32_t val;
      if (COMPACT && !(r.flags & ROW_IRREGULAR)) {
        unsigned rd;
        const CfoEnt e = cfo_pick<NT>(g.cfo + r.off, r.deg, m, rd, g.cfo_reload != 0);
        val = e.id; r = imp_link_row(e.link);
      } else {
        const float u = (float)m * (1.0f / 16777216.0f);
        if (r.flags & ROW_IRREGULAR) {
          const int32_t k = lane_pick_sequential(g.ent + r.off, r.deg, nobias, u);
          if (COMPACT) {                                 // only the compact table exists: its links are valid for every row
            const CfoEnt e = g.cfo[r.off + k];
            val = e.id; r = imp_link_row(e.link);
          } else {
            const FoEnt e = g.fo[r.off + k];
            val = e.id; r.off = e.noff; r.deg = e.ndeg; r.flags = e.nflags;
          }
        } else {
          unsigned rd; int32_t k;
          const FoEnt e = fo_pick<NT>(g.fo + r.off, r.deg, u, k, rd);
          val = e.id; r.off = e.noff; r.deg = e.ndeg; r.flags = e.nflags;
        }
      }
      const uint32_t vs = (uint32_t)((int64_t)val - g.vmin);
      out[(int64_t)s * R] = vs == seed_slot ? IMP_NONE : vs;
    }
    for (; s < L; ++s) out[(int64_t)s * R] = IMP_NONE;
  }
}

__device__ inline unsigned long long imp_wave_max_u64(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) { const unsigned long long x = __shfl_xor(v, o); v = x > v ? x : v; }
  return v;
}

template <int N>
__global__ __launch_bounds__(64) void k_imp_topk(GraphView g, const uint32_t *__restrict__ visits, int64_t n_seeds, int32_t RL, int32_t T,
                                                 int32_t *__restrict__ ids, int32_t *__restrict__ counts, int32_t *__restrict__ total) {
  static_assert(N >= 64 && N <= IMP_MAX_VISITS && (N & (N - 1)) == 0, "a power of two, one position per lane at least");
  constexpr int U = 4;                                  // compare-exchanges a lane has in flight: their LDS round trips overlap
  __shared__ uint32_t a[N];
  __shared__ unsigned short cnt[N];
  const int lane = (int)threadIdx.x;
  for (int64_t b = blockIdx.x; b < n_seeds; b += gridDim.x) {          // (block-uniform: every barrier below is met by the whole block)
    const uint32_t *row = visits + b * (int64_t)RL;
    int32_t live = 0;                                     // (wave-uniform) the visits of this seed
    uint32_t best_c = 0u, best_slot = 0u; int best_t = 0, passes = 0;
    if constexpr (N == 64) {
      // ---- at most one visit per lane: the whole of it in registers.  The bitonic network by shuffles (a lane keeps the smaller of
      // the pair when it is the lower one of an ascending pair or the upper one of a descending pair), the run tails by one more.
      uint32_t v = lane < RL ? row[lane] : IMP_NONE;
      live = __popcll(__ballot(v != IMP_NONE));
      for (int k = 2; k <= 64; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
          const uint32_t o = (uint32_t)__shfl_xor((int)v, j);
          v = (((lane & j) == 0) == ((lane & k) == 0)) ? min(v, o) : max(v, o);
        }
      }
      const uint32_t nxt = (uint32_t)__shfl_down((int)v, 1);
      const bool tail = lane == 63 || nxt != v;
      const unsigned long long below = __ballot(tail) & ((1ull << lane) - 1ull);
      const int32_t prev = below ? 63 - (int)__builtin_clzll(below) : -1;
      best_c = (tail && v != IMP_NONE) ? (uint32_t)(lane - prev) : 0u;
      best_slot = v;
    } else {
      // ---- the visits, compacted: a walk with restart leaves most of its L places empty, and only what is there is sorted
      for (int i0 = 0; i0 < RL; i0 += 64) {
        const uint32_t v = i0 + lane < RL ? row[i0 + lane] : IMP_NONE;
        const unsigned long long there = __ballot(v != IMP_NONE);
        if (v != IMP_NONE) a[live + __popcll(there & ((1ull << lane) - 1ull))] = v;
        live += __popcll(there);
      }
      int n = 64;                                           // the sorted length: the power of two >= live (<= N, as live <= R * L)
      while (n < live) n <<= 1;
      for (int i = live + lane; i < n; i += 64) a[i] = IMP_NONE;
      passes = n >> 6;
      __syncthreads();
      // ---- ascending bitonic sort: stage (k, j) compares a[i] with a[i | j], i without bit j; the direction is bit k of i.  The pairs
      // of a stage are disjoint: U of them are loaded before the first is stored.
      for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
          for (int p0 = lane; p0 < n / 2; p0 += 64 * U) {
            uint32_t x[U], y[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
              const int p = p0 + 64 * u, i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
              if (p < n / 2) { x[u] = a[i]; y[u] = a[i | j]; }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
              const int p = p0 + 64 * u, i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
              if (p < n / 2 && (x[u] > y[u]) == ((i & k) == 0)) { a[i] = y[u]; a[i | j] = x[u]; }
            }
          }
          __syncthreads();
        }
      }
      // ---- run tails and their counts; every lane's best own position
      int32_t last_tail = -1;                               // (wave-uniform) the last tail of the passes so far
      for (int t = 0; t < passes; ++t) {
        const int i = 64 * t + lane;
        const uint32_t v = a[i];
        const bool tail = i == n - 1 || a[i + 1] != v;
        const unsigned long long tails = __ballot(tail);
        const unsigned long long below = tails & ((1ull << lane) - 1ull);
        const int32_t prev = below ? 64 * t + 63 - (int)__builtin_clzll(below) : last_tail;
        const uint32_t c = (tail && v != IMP_NONE) ? (uint32_t)(i - prev) : 0u;
        cnt[i] = (unsigned short)c;                          // (c <= 4096)
        if (c > best_c) { best_c = c; best_t = t; best_slot = v; }
        if (tails) last_tail = 64 * t + 63 - (int)__builtin_clzll(tails);
      }
    }
    // ---- T times the wave's maximum of (count, -slot); a lane reads and writes only the cnt[] it owns
    uint32_t my_slot = 0u, my_c = 0u;                     // lane t: the t-th of the result
    for (int t = 0; t < T; ++t) {
      const unsigned long long key = ((unsigned long long)best_c << 32) | (uint32_t)~best_slot;
      const unsigned long long mx = imp_wave_max_u64(key);
      if ((mx >> 32) == 0ull) break;                      // nothing left: the rest is padding
      if (lane == t) { my_c = (uint32_t)(mx >> 32); my_slot = ~(uint32_t)mx; }
      if (key == mx) {                                    // (one lane: a slot has one tail)
        if constexpr (N > 64) cnt[64 * best_t + lane] = 0;
        best_c = 0u; best_slot = 0u; best_t = 0;
        for (int tt = 0; tt < passes; ++tt) {             // (N == 64: a lane owns one position, nothing is left)
          const uint32_t c = cnt[64 * tt + lane];
          if (c > best_c) { best_c = c; best_t = tt; }
        }
        if (best_c) best_slot = a[64 * best_t + lane];
      }
    }
    if (lane < T) {
      int32_t id = -1;
      if (my_c && (int64_t)my_slot < g.n_slots) id = g.orig_id ? g.orig_id[my_slot] : (int32_t)((int64_t)my_slot + g.vmin);
      else my_c = 0u;
      ids[b * T + lane] = id;
      counts[b * T + lane] = (int32_t)my_c;
    }
    if (total && lane == 0) total[b] = live;
    if constexpr (N > 64) __syncthreads();                // the next seed's load overwrites a[]
  }
}

}  // namespace

int64_t importance_neighbors(srw_handle *h, const int32_t *d_seeds, int64_t n_seeds, const srw_importance_params &ip, int32_t *d_ids,
                             int32_t *d_counts, int32_t *d_total) {
  Graph &g = h->g;
  hipStream_t st = h->stream;
  const bool no_compact = (ip.flags & SRW_IMP_NO_COMPACT) != 0;
  // the tables of a p = q = 1 walk, built as that walk builds them (SRW_IMP_NO_COMPACT: as under SRW_WALK_NO_COMPACT)
  build_first_order_tables(h, no_compact);
  const bool compact = g.has_cfo && !no_compact;
  if (!compact && !g.has_fo) throw Error(SRW_ERR_INVALID, "srw_importance_neighbors: no first-order table after the build");
  // the load policy launch_walk chooses for these records: L1-bypassing once the table is far beyond L2 + Infinity Cache
  const bool nt = (size_t)g.n_entries * (compact ? sizeof(CfoEnt) : sizeof(FoEnt)) > ((size_t)2 << 30);
  const GraphView gv = g.view();
  const int32_t R = ip.num_walks, L = ip.walk_length, T = ip.top;
  const int32_t RL = R * L;                              // (<= IMP_MAX_VISITS: api.cpp)
  int N = 64;
  while (N < RL) N <<= 1;
  const int64_t chunk = std::min<int64_t>(n_seeds, (int64_t)(IMP_SCRATCH_BYTES / ((size_t)RL * 4u)));
  h->imp_visits.ensure((size_t)chunk * (size_t)RL);
  h->sgns_skipped.ensure(1);
  SRW_HIP(hipMemsetAsync(h->sgns_skipped.p, 0, 8, st));
  for (int64_t b0 = 0; b0 < n_seeds; b0 += chunk) {      // (no host round trip between the chunks: the stream orders the scratch's reuse)
    const int64_t nb = std::min<int64_t>(chunk, n_seeds - b0), n_walks = nb * R;
    const dim3 wgrid((unsigned)std::min<int64_t>((n_walks + TPB - 1) / TPB, (int64_t)h->n_cus * IMP_BLOCKS_PER_CU));
#define SRW_LAUNCH_IMP(NTV, CP)                                                                                                   \
  hipLaunchKernelGGL((k_imp_walk<NTV, CP>), wgrid, dim3(TPB), 0, st, gv, d_seeds + b0, h->imp_visits.p, n_walks, R, L,            \
                     ip.base + (uint32_t)b0, ip.seed, ip.epoch, ip.restart_m, (int32_t)((ip.flags & SRW_IMP_KEEP_SEED) != 0), h->sgns_skipped.p)
    if (compact) { if (nt) SRW_LAUNCH_IMP(true, true); else SRW_LAUNCH_IMP(false, true); }
    else         { if (nt) SRW_LAUNCH_IMP(true, false); else SRW_LAUNCH_IMP(false, false); }
#undef SRW_LAUNCH_IMP
    SRW_HIP(hipGetLastError());
    const dim3 tgrid((unsigned)std::min<int64_t>(nb, (int64_t)h->n_cus * std::min(32, IMP_LDS_PER_CU / (6 * N))));
#define SRW_LAUNCH_TOPK(NV)                                                                                                       \
  hipLaunchKernelGGL((k_imp_topk<NV>), tgrid, dim3(64), 0, st, gv, h->imp_visits.p, nb, RL, T, d_ids + b0 * T, d_counts + b0 * T,  \
                     d_total ? d_total + b0 : nullptr)
    switch (N) {
      case 64: SRW_LAUNCH_TOPK(64); break;
      case 128: SRW_LAUNCH_TOPK(128); break;
      case 256: SRW_LAUNCH_TOPK(256); break;
      case 512: SRW_LAUNCH_TOPK(512); break;
      case 1024: SRW_LAUNCH_TOPK(1024); break;
      case 2048: SRW_LAUNCH_TOPK(2048); break;
      default: SRW_LAUNCH_TOPK(4096); break;
    }
#undef SRW_LAUNCH_TOPK
    SRW_HIP(hipGetLastError());
  }
  unsigned long long unknown = 0;
  SRW_HIP(hipMemcpyAsync(&unknown, h->sgns_skipped.p, 8, hipMemcpyDeviceToHost, st));
  SRW_HIP(hipStreamSynchronize(st));
  return (int64_t)unknown;
}

}  // namespace srw
