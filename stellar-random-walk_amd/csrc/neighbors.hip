// neighbors.hip — the layered fan-out neighbour sample of a mini-batch of seeds (gfx950): srw_sample_neighbors (include/stellar_rw.h,
// DESIGN §7h).  No reference counterpart: the reference only walks.  The weighted draw is RandomSample.sample
// (M/algorithm/RandomSample.scala:12-25) through the tables a p = q = 1 walk builds; nothing else is built or kept.
//
// One launch per layer; layer l [n_seeds][F_l] reads layer l-1 [n_seeds][F_{l-1}] (layer 0: the seeds), F_l = F_{l-1} * f.  Element
// idx = b * F_l + j of layer l has the parent idx / f of layer l-1 and the word philox4x32_10((b, j, l, epoch), (seed, 64))[0].
//
//   k_nbr_replace<NT, COMPACT>   with replacement: one output element per lane, grid-stride over the 64-bit element index; the f lanes
//                                that share a parent load one address.  vertex_slot, the row descriptor, then the three arms of
//                                k_walk_first_order's step (walk_kernels.hip): cfo_pick over the 16-byte lattice records on regular rows
//                                (COMPACT), fo_pick over the 32-byte records otherwise, lane_pick_sequential on ROW_IRREGULAR rows.  The
//                                lanes do not depend on each other and nothing is staged: no LDS.  The picked record's link (the child's
//                                row descriptor) is NOT carried to the next layer: every layer looks its parents up again (one row read,
//                                16 bytes shared by the parent's f lanes) — the side buffer was not built, so there is nothing to A/B.
//   k_nbr_distinct<G>            without replacement: one parent per group of G lanes (G = the power of two >= f: 1 .. 64, 64 / G
//                                parents per wave), lane i of the group owns child i.  deg <= f copies the row in row order, then -1.
//                                Otherwise Floyd's algorithm: every lane computes its own t_i (the words are independent per child), then
//                                f - 1 rounds — round i broadcasts t_i inside the group, the lanes below i compare it with the position
//                                they ended up with, one ballot masked to the group decides "taken -> J".  Reads ids32 where a
//                                unit-weight graph has it, ent otherwise.
// Grid: at most NBR_BLOCKS_PER_CU blocks of 256 per CU (16 waves per CU: ~260 000 independent requests in flight on the chip, several
// times what the memory system's latency x request rate asks for); more elements than that take further trips of the grid-stride loop.
#include <algorithm>
#include <string>

#include "engine.h"
#include "sampling.h"
#include "walk_shared.h"

namespace srw {
namespace {

#ifndef SRW_NBR_BLOCKS_PER_CU                          // experiment builds: make variant NAME=b8 EXTRA=-DSRW_NBR_BLOCKS_PER_CU=8
#define SRW_NBR_BLOCKS_PER_CU 4
#endif
constexpr int NBR_BLOCKS_PER_CU = SRW_NBR_BLOCKS_PER_CU;
constexpr uint32_t NBR_KEY = 64u;                      // Philox key word 1 of this stream (0 .. 32: the walk and the negatives)

__device__ inline uint32_t nbr_word(uint32_t seed, uint32_t epoch, uint32_t b, uint32_t j, uint32_t layer) {
  uint32_t o[4];
  philox4x32_10(b, j, layer, epoch, seed, NBR_KEY, o);
  return o[0];
}

// The row of a parent id as a tensor spells it (the input's id): false — and an empty row — for -1 and for an id that is no present
// vertex.  The id reaches no address before vertex_slot has checked it.
__device__ inline bool nbr_parent_row(const GraphView &g, int32_t pid, Row &r) {
  r.off = 0; r.deg = 0; r.flags = 0;
  if (pid == -1) return false;
  const int64_t s = vertex_slot(pid, g.rows, g.orig_id, g.n_slots, g.vmin);
  if (s >= g.n_slots) return false;
  r = g.rows[s];
  return true;
}

// an id as the engine holds it (slot + vmin) -> the input's id
__device__ inline int32_t nbr_out_id(const GraphView &g, int32_t id) { return g.orig_id ? g.orig_id[id - g.vmin] : id; }

template <bool NT, bool COMPACT>
__global__ __launch_bounds__(TPB) void k_nbr_replace(GraphView g, const int32_t *__restrict__ parents, int32_t *__restrict__ out,
                                                     int64_t total, int64_t F, int32_t f, uint32_t layer, uint32_t seed, uint32_t epoch,
                                                     unsigned long long *unknown) {
  const int64_t Fp = F / f;                              // row length of the parents' layer
  Bias nobias; nobias.second_order = false; nobias.need_member = false; nobias.p = nobias.q = 1.0f;
  nobias.prev = 0; nobias.prev_sids = nullptr; nobias.prev_deg = 0; nobias.vmin = g.vmin;
  for (int64_t idx = blockIdx.x * (int64_t)TPB + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * TPB) {
    const int64_t b = idx / F;
    const uint32_t j = (uint32_t)(idx - b * F);
    const int32_t pid = parents[b * Fp + (int64_t)(j / (uint32_t)f)];
    Row r;
    const bool present = nbr_parent_row(g, pid, r);
    if (unknown && !present && j == 0u) atomicAdd(unknown, 1ull);      // (layer 1 only: j == 0 is the seed's first child)
    int32_t val = -1;
    if (r.deg > 0) {
      const uint32_t m = nbr_word(seed, epoch, (uint32_t)b, j, layer) >> 8;
      if (COMPACT && !(r.flags & ROW_IRREGULAR)) {
        unsigned rd;
        val = cfo_pick<NT>(g.cfo + r.off, r.deg, m, rd, g.cfo_reload != 0).id;
      } else {
        const float u = (float)m * (1.0f / 16777216.0f);
        if (r.flags & ROW_IRREGULAR) {
          val = g.ent[r.off + lane_pick_sequential(g.ent + r.off, r.deg, nobias, u)].id;
        } else {
          unsigned rd; int32_t k;
          val = fo_pick<NT>(g.fo + r.off, r.deg, u, k, rd).id;
        }
      }
      val = nbr_out_id(g, val);
    }
    out[idx] = val;
  }
}

template <int G>
__global__ __launch_bounds__(TPB) void k_nbr_distinct(GraphView g, const int32_t *__restrict__ parents, int32_t *__restrict__ out,
                                                      int64_t n_parents, int64_t Fp, int32_t f, uint32_t layer, uint32_t seed,
                                                      uint32_t epoch, unsigned long long *unknown) {
  constexpr int GPW = 64 / G;                            // parents per wave
  const int lane = lane_id();
  const int sub = lane & (G - 1), gbase = lane & ~(G - 1);
  const unsigned long long gmask = (G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull)) << gbase;
  const int64_t wave = (blockIdx.x * (int64_t)TPB + threadIdx.x) >> 6, n_waves = (int64_t)gridDim.x * (TPB / 64);
  for (int64_t p0 = wave * GPW; p0 < n_parents; p0 += n_waves * GPW) {   // (wave-uniform: the rounds below are the whole wave's)
    const int64_t p = p0 + (lane / G);
    const bool live = p < n_parents;
    Row r;
    const bool present = nbr_parent_row(g, live ? parents[p] : -1, r);
    if (unknown && live && !present && sub == 0) atomicAdd(unknown, 1ull);   // (layer 1 only: a parent is a seed)
    const int32_t deg = r.deg;
    const bool floyd = deg > f;                          // the same in every lane of a group
    int32_t pos = -1, t = -1, J = 0;                     // pos: the row position of child `sub`, -1 = none
    if (sub < f) {
      if (!floyd) pos = sub < deg ? sub : -1;            // the row in row order, then -1
      else {
        const int64_t b = p / Fp;
        const uint32_t j = (uint32_t)(p - b * Fp) * (uint32_t)f + (uint32_t)sub;
        J = deg - f + sub;
        t = (int32_t)(((uint64_t)nbr_word(seed, epoch, (uint32_t)b, j, layer) * (uint64_t)(uint32_t)(J + 1)) >> 32);
        pos = t;
      }
    }
    if (__ballot(floyd)) {
      for (int i = 1; i < f; ++i) {                      // child i: taken by an earlier child of this parent -> J
        const int32_t ti = __shfl(t, gbase + i);
        const unsigned long long hit = __ballot(floyd && sub < i && pos == ti) & gmask;
        if (floyd && sub == i && hit) pos = J;
      }
    }
    if (live && sub < f) {
      int32_t val = -1;
      if (pos >= 0) val = nbr_out_id(g, g.ids32 ? g.ids32[r.off + pos] : g.ent[r.off + pos].id);
      out[p * f + sub] = val;
    }
  }
}

}  // namespace

int64_t sample_neighbors(srw_handle *h, const int32_t *d_seeds, int64_t n_seeds, const int32_t *fanouts, int32_t n_layers,
                         const srw_neighbor_params &np, int32_t *const *d_layers) {
  Graph &g = h->g;
  hipStream_t st = h->stream;
  const bool replace = np.replace != 0;
  // the tables of a p = q = 1 walk, built as that walk builds them (SRW_NBR_NO_COMPACT: as under SRW_WALK_NO_COMPACT)
  if (replace) build_first_order_tables(h, (np.flags & SRW_NBR_NO_COMPACT) != 0);
  const bool compact = replace && g.has_cfo && !(np.flags & SRW_NBR_NO_COMPACT);
  if (replace && !compact && !g.has_fo) throw Error(SRW_ERR_INVALID, "srw_sample_neighbors: no first-order table after the build");
  // the load policy launch_walk chooses for these records: L1-bypassing once the table is far beyond L2 + Infinity Cache
  const bool nt = (size_t)g.n_entries * (compact ? sizeof(CfoEnt) : sizeof(FoEnt)) > ((size_t)2 << 30);
  const GraphView gv = g.view();
  h->sgns_skipped.ensure(1);
  SRW_HIP(hipMemsetAsync(h->sgns_skipped.p, 0, 8, st));
  const int64_t max_blocks = (int64_t)h->n_cus * NBR_BLOCKS_PER_CU;
  int64_t Fp = 1;
  const int32_t *parents = d_seeds;
  for (int32_t l = 1; l <= n_layers; ++l) {
    const int32_t f = fanouts[l - 1];
    const int64_t F = Fp * f, n_parents = n_seeds * Fp, total = n_seeds * F;
    unsigned long long *unknown = l == 1 ? h->sgns_skipped.p : nullptr;
    int32_t *out = d_layers[l - 1];
    if (replace) {
      const dim3 grid((unsigned)std::min<int64_t>((total + TPB - 1) / TPB, max_blocks));
#define SRW_LAUNCH_NBR(NTV, CP)                                                                                                  \
  hipLaunchKernelGGL((k_nbr_replace<NTV, CP>), grid, dim3(TPB), 0, st, gv, parents, out, total, F, f, (uint32_t)l, np.seed, np.epoch, unknown)
      if (compact) { if (nt) SRW_LAUNCH_NBR(true, true); else SRW_LAUNCH_NBR(false, true); }
      else         { if (nt) SRW_LAUNCH_NBR(true, false); else SRW_LAUNCH_NBR(false, false); }
#undef SRW_LAUNCH_NBR
    } else {
      int G = 1;
      while (G < f) G <<= 1;
      const int64_t per_block = (TPB / 64) * (64 / G);
      const dim3 grid((unsigned)std::min<int64_t>((n_parents + per_block - 1) / per_block, max_blocks));
#define SRW_LAUNCH_NBD(GV)                                                                                                       \
  hipLaunchKernelGGL((k_nbr_distinct<GV>), grid, dim3(TPB), 0, st, gv, parents, out, n_parents, Fp, f, (uint32_t)l, np.seed, np.epoch, unknown)
      switch (G) {
        case 1: SRW_LAUNCH_NBD(1); break;
        case 2: SRW_LAUNCH_NBD(2); break;
        case 4: SRW_LAUNCH_NBD(4); break;
        case 8: SRW_LAUNCH_NBD(8); break;
        case 16: SRW_LAUNCH_NBD(16); break;
        case 32: SRW_LAUNCH_NBD(32); break;
        default: SRW_LAUNCH_NBD(64); break;
      }
#undef SRW_LAUNCH_NBD
    }
    SRW_HIP(hipGetLastError());
    parents = out; Fp = F;
  }
  unsigned long long unknown = 0;
  SRW_HIP(hipMemcpyAsync(&unknown, h->sgns_skipped.p, 8, hipMemcpyDeviceToHost, st));
  SRW_HIP(hipStreamSynchronize(st));
  return (int64_t)unknown;
}

}  // namespace srw
