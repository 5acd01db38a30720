// shard_kernels.hip — the vertex-sharded multi-GPU walk (gfx950): one super-step at a time, the k_sh_* kernels and the host side of one rank.
// Vertex-sharded walk (SURVEY §8e option 2; replaces transferWalkersToTheirPartitions, RandomWalk.scala:92-93,186-192,
// and UniformRandomWalk.prepareWalkersToTransfer, UniformRandomWalk.scala:103-112).
//
// A walker standing on v is processed by owner(v); its PATH lives on its home rank = owner(source).  What moves between
// ranks each super-step is fixed-size records in fixed-capacity CHUNKS, one chunk per (sender, receiver) pair:
//     chunk = { u32 n_walkers, n_rets, 0, 0 } | WWalker[cap_w] {lw, src, prev, curr} | WRet[cap_r] {lw, v}
// 16 + 8 = 24 bytes per walker-step on the wire (the reference ships the whole path so far and N(prev) with every walker,
// RandomWalk.scala:135).  lw = (local index of the source vertex on its home rank) * batch + (walk iteration inside the
// batch): the home rank's path row, and lw % batch is the RNG's iteration word.  Every sampled vertex goes home at once as
// an 8-byte return; its path slot is IMPLICIT: a return produced by super-step s belongs to slot s (the receiver applies
// the returns of the chunk it got after super-step s).  A return with the top bit of lw set is a death notice (the walker
// stopped before sampling slot s: its path has s entries): lens start at walk_length + 2 and only walkers that stop early
// are corrected.  On a linked p = q = 1 walk prev | curr << 32 is the row link of the vertex the walker stands on.
// (Round 2 carried the last three vertices inside a 32-byte walker and returned four slots at a time as 24 bytes: 38 bytes
// per walker-step — the exchange, not the kernels, bounded a shard on xGMI)
// A rank's receive buffer is `world` chunks (one per sender), its send side is `world` destination pointers — the
// local send buffer (one equal-split all_to_all_single moves it, distributed.py) or, inside one process, the peers'
// receive buffers themselves (xGMI peer stores, cluster.cpp).
// Everything is sized and counted on the device: NO host synchronisation per super-step; an overflowing chunk drops
// its surplus and raises a flag the host reads once per batch (the batch is then redone with more slack).
//   k_sh_seed    : the rank's own walkers, spread over the chunks of its receive buffer; path slot 0, lens = L + 2
//   k_sh_apply   : returns of the previous super-step -> their path slot; death notices -> lens
//   k_sh_step(_fo): sample every incoming walker once into `scratch` (kind says what the bucket kernel must emit), count
//                  the block's survivors per destination owner and the returns per home rank in LDS -> blk[b][2 * world]
//   k_sh_offsets : one block: scan of blk over the blocks -> every block's write cursors; chunk headers
//   k_sh_bucket  : re-reads the slice, writes walkers to chunk[owner(next)] and path returns to chunk[home(src)]
// The general kernel keeps one wave per record and the same samplers as k_walk_general (bit-identical paths for any
// world, asserted against the oracle).
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "engine.h"
#include "sampling.h"
#include "walk_shared.h"

namespace srw {
namespace {
__device__ inline Bias make_bias(const GraphView &g, float p, float q, int32_t prev, bool second_order) {
  Bias b;
  b.p = p; b.q = q; b.prev = prev; b.second_order = second_order;
  b.need_member = second_order && (q != 1.0f);
  b.prev_sids = nullptr; b.prev_deg = 0; b.vmin = g.vmin;
  if (b.need_member) {   // N(prev) through the membership structure (replicated on every shard)
    int64_t s = (int64_t)prev - g.vmin;
    if (s >= 0 && s < g.n_slots) { Row r = g.mrows[s]; b.prev_sids = g.msids + r.off; b.prev_deg = r.deg; b.prev_hub = r.flags >> ROW_HUB_SHIFT; }
  }
  return b;
}

__device__ inline void shard_return_home(const ShardIO &io, const SWalker &w, int32_t step) {
  if (w.kind == SK_DEAD) io.lens[w.lw] = step;
  else io.pt[(int64_t)step * io.n_rows + w.lw] = w.v;
}

__device__ inline void block_flush_counters(DevCounters *ctr, unsigned long long *red, unsigned long long steps,
                                            unsigned long long dead, unsigned long long degc, unsigned long long degp,
                                            unsigned long long reads, unsigned long long fb) {
  // red: 6 words of LDS, zeroed before the block's work; one global atomic per counter per BLOCK
  steps = wave_sum_u64(steps); dead = wave_sum_u64(dead); degc = wave_sum_u64(degc);
  degp = wave_sum_u64(degp); reads = wave_sum_u64(reads); fb = wave_sum_u64(fb);
  if (lane_id() == 0) {
    if (steps) atomicAdd(&red[0], steps);
    if (dead) atomicAdd(&red[1], dead);
    if (degc) atomicAdd(&red[2], degc);
    if (degp) atomicAdd(&red[3], degp);
    if (reads) atomicAdd(&red[4], reads);
    if (fb) atomicAdd(&red[5], fb);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (red[0]) atomicAdd(&ctr->steps, red[0]);
    if (red[1]) atomicAdd(&ctr->dead_ends, red[1]);
    if (red[2]) atomicAdd(&ctr->sum_deg_curr, red[2]);
    if (red[3]) atomicAdd(&ctr->sum_deg_prev, red[3]);
    if (red[4]) atomicAdd(&ctr->ent_reads, red[4]);
    if (red[5]) atomicAdd(&ctr->fallbacks, red[5]);
  }
}

// per-block slice of n records in units of `unit` records (TPB for the per-lane kernels, TPB / 64 for one wave per record)
__device__ inline void shard_slice(uint32_t n, uint32_t unit, uint32_t &lo, uint32_t &hi) {
  uint32_t per = (n + gridDim.x - 1) / gridDim.x;
  per = (per + unit - 1) / unit * unit;
  const uint64_t l = (uint64_t)blockIdx.x * per, h = l + per;
  lo = (uint32_t)(l < n ? l : n); hi = (uint32_t)(h < n ? h : n);
}

__device__ inline SWalker shard_dead(const SWalker &wk) { SWalker d = wk; d.kind = SK_DEAD; return d; }
__device__ inline WWalker shard_wire_of(const SWalker &w) { WWalker o; o.lw = w.lw; o.src = w.src; o.prev = w.prev; o.curr = w.curr; return o; }
__device__ inline WRet shard_ret_of(const SWalker &w) {
  WRet r;
  r.lw = w.kind == SK_DEAD ? (int32_t)((uint32_t)w.lw | 0x80000000u) : w.lw;
  r.v = w.kind == SK_DEAD ? 0 : w.v;
  return r;
}

// linked walkers (k_sh_step_cfo): prev | curr << 32 = the link of the vertex the walker stands on, laid out as CfoEnt::link
__device__ inline uint64_t shard_link_of(const Row &r) {
  return ((uint64_t)r.off & CFO_NOFF_MASK) | ((uint64_t)(uint32_t)min(r.deg, (int32_t)CFO_NDEG_MAX) << 40) |
         ((uint64_t)((r.flags & ROW_IRREGULAR) != 0) << 63);
}
// A shard's own seeds must fit the chunks of its receive buffer: n_local * batch / world per chunk against a capacity sized
// from nVertices / world^2 — skewed ownership (SRW_CFG_OWNER_FROM_PARTITIONS with fewer partitions than GPUs) breaks that,
// so the surplus is dropped and the overflow flag raised like everywhere else (the batch is redone with more slack).
__global__ void k_sh_seed(const int32_t *__restrict__ verts, int64_t n_local, ShardIO io, char *recv_w,
                          int32_t *__restrict__ paths, int32_t *__restrict__ lens, int64_t stride,
                          const Row *__restrict__ link_rows, int32_t vmin, uint32_t *overflow) {
  const int64_t n = n_local * io.batch;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t src = verts[i / io.batch];
    WWalker w; w.lw = (int32_t)i; w.src = src; w.prev = src; w.curr = src;
    if (link_rows) { const uint64_t l = shard_link_of(link_rows[(int64_t)src - vmin]); w.prev = (int32_t)(uint32_t)l; w.curr = (int32_t)(uint32_t)(l >> 32); }
    const int c = (int)(i % io.world);
    if (i / io.world < (int64_t)io.cap_w) reinterpret_cast<WWalker *>(recv_w + c * io.chunk_bytes + 16)[i / io.world] = w;
    paths[i] = src;                   // slot 0 of the slot-major staging [stride][n] (k_sh_apply)
    lens[i] = (int32_t)stride;        // full length unless a death notice says otherwise (k_sh_apply)
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < io.world) {
    const int c = (int)threadIdx.x;
    uint32_t *h = reinterpret_cast<uint32_t *>(recv_w + c * io.chunk_bytes);
    const int64_t mine = (n - c + io.world - 1) / io.world;
    if (mine > (int64_t)io.cap_w) atomicOr(overflow, 1u);
    h[0] = (uint32_t)(mine < (int64_t)io.cap_w ? mine : (int64_t)io.cap_w); h[1] = 0u; h[2] = 0u; h[3] = 0u;
  }
}

// returns of the previous super-step: each one is path slot `slot` of its walker; death notices set lens.
// The home rank stages its paths SLOT-MAJOR, pt[slot][row]: the 4-byte stores of one super-step — one per walker, in the
// order the returns arrive — then fall into one contiguous n_rows * 4 B row that the caches absorb (L2 + Infinity Cache) and
// write back as full lines; into the final [row][L + 2] matrix they were one partial 64-byte sector each, and k_sh_apply
// cost as much as the sampling kernel (s15: 1.94 ms vs 1.90 ms per super-step of 35.5 M walkers).  k_sh_transpose turns
// the staging into the final layout once per batch (two streaming passes over the batch's paths).
__global__ void k_sh_apply(ShardIO io, int32_t *__restrict__ pt, int32_t *__restrict__ lens, int64_t n_rows, int32_t slot) {
  for (int c = 0; c < io.world; ++c) {
    const uint32_t n = min(chunk_hdr(io.recv, io.chunk_bytes, c)[1], (uint32_t)io.cap_r);
    const WRet *r = chunk_rets(io.recv, io.chunk_bytes, io.cap_w, c);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
      const WRet x = r[i];
      if (x.lw < 0) lens[x.lw & 0x7FFFFFFF] = slot;             // death notice: the walker stopped with `slot` entries
      else pt[(int64_t)slot * n_rows + x.lw] = x.v;
    }
  }
}

// pt[slot][row] -> paths[row][slot], -1 beyond the row's length: tiles of 64 rows x 16 slots through LDS, 256-byte reads,
// 64-byte runs per row on the way out.
__global__ __launch_bounds__(TPB) void k_sh_transpose(const int32_t *__restrict__ pt, const int32_t *__restrict__ lens, int64_t n_rows,
                                                      int64_t stride, int32_t *__restrict__ paths) {
  __shared__ int32_t tile[16][64 + 1];
  const int t = threadIdx.x;
  for (int64_t w0 = (int64_t)blockIdx.x * 64; w0 < n_rows; w0 += (int64_t)gridDim.x * 64) {
    const int64_t wr = w0 + (t >> 2);
    const int32_t len = wr < n_rows ? lens[wr] : 0;
    for (int64_t s0 = 0; s0 < stride; s0 += 16) {
#pragma unroll
      for (int pass = 0; pass < 4; ++pass) {
        const int64_t sl = s0 + pass * 4 + (t >> 6), w = w0 + (t & 63);
        tile[pass * 4 + (t >> 6)][t & 63] = (sl < stride && w < n_rows) ? pt[sl * n_rows + w] : -1;
      }
      __syncthreads();
      if (wr < n_rows) {
        const int c0 = (t & 3) * 4;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int64_t sl = s0 + c0 + c;
          if (sl < stride) paths[wr * stride + sl] = sl < len ? tile[c0 + c][t >> 2] : -1;
        }
      }
      __syncthreads();
    }
  }
}

// todo != null: only the records listed there (those k_sh_step_tab found no table for); k_sh_scatter then buckets the
// whole scratch array, so no per-block counts are produced.
__global__ __launch_bounds__(TPB, 4) void k_sh_step(GraphView g, ShardIO io, int32_t first_walk, int32_t step, int32_t last,
                                                    RngSpec rng, float p, float q, SWalker *__restrict__ scratch,
                                                    uint32_t *__restrict__ blk, DevCounters *ctr,
                                                    const uint32_t *__restrict__ todo, const unsigned long long *todo_n) {
  __shared__ __attribute__((aligned(16))) uint32_t bitmap[TPB / 64][BINNED_LDS_WORDS];
  __shared__ uint32_t cnt[2 * SHARD_MAX_WORLD], pre[SHARD_MAX_WORLD + 1];
  __shared__ unsigned long long red[6];
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  if (threadIdx.x < 2 * SHARD_MAX_WORLD) cnt[threadIdx.x] = 0u;
  if (threadIdx.x < 6) red[threadIdx.x] = 0ull;
  const uint32_t n_in = shard_in_prefix(io, pre);          // contains the __syncthreads() cnt / red need
  Member mem; mem.mode = 0; mem.bm = bitmap[wv]; mem.seg_base = 0;
  unsigned long long steps = 0, dead = 0, degc = 0, degp = 0, fb = 0;
  uint32_t n_strat[8] = {0, 0, 0, 0, 0, 0, 0, 0};           // SRW_STRAT_* 0 .. 7 (lane 0 counts)
  uint32_t lo, hi;
  shard_slice(n_in, TPB / 64, lo, hi);
  uint32_t t_step = TPB / 64;
  if (todo) { lo = blockIdx.x * (TPB / 64); hi = (uint32_t)*todo_n; t_step = gridDim.x * (TPB / 64); }
  for (uint32_t ti = lo + wv; ti < hi; ti += t_step) {     // one wave per record
    const uint32_t ri = todo ? todo[ti] : ti;
    const SWalker wk = shard_in_record(io, pre, ri);
    const Row *rp = row_of(g, wk.curr);
    Row r; r.off = 0; r.deg = 0; r.flags = 0;
    if (rp) r = *rp;
    if (r.deg == 0) {                                  // dead end (or a source without neighbors): tell the home rank the length
      if (lane == 0) {
        scratch[ri] = shard_dead(wk);
        const int32_t hm = owner_of_tab(wk.src, io.world, g.owner_tab, g.vmin, g.n_slots);
        if (hm != io.rank) atomicAdd(&cnt[SHARD_MAX_WORLD + hm], 1u);
      }
      if (step > 1) dead += (lane == 0);
      continue;
    }
    const uint32_t iter = (uint32_t)(first_walk + wk.lw % io.batch);
    Bias b = make_bias(g, p, q, wk.prev, step > 1);
    float u = draw_uniform(rng, iter, (uint32_t)rng_source(g, wk.src), (uint32_t)step);
    unsigned f = 0, sv = 0;
    int32_t k = -1, nid = 0;                         // same routing as k_walk_general (no per-edge tables on a shard)
    unsigned which = SRW_STRAT_SCAN;
    if (!b.need_member) { k = wave_pick_prefix(g, r, (int64_t)wk.curr - g.vmin, b, mem.bm, u, f, sv); if (k >= 0) which = SRW_STRAT_PREFIX; }
    else {
      unsigned long long ab = 0; unsigned su = 0;
      k = wave_pick_binned(g, r, (int64_t)wk.curr - g.vmin, b, mem.bm, u, f, sv, 0, false, mem, ab, su, nid);
      if (k >= 0) which = su == 1 ? SRW_STRAT_P1 : su == 2 ? SRW_STRAT_P2 : su == 4 ? SRW_STRAT_P3 : SRW_STRAT_W;
    }
    if (k < 0) k = wave_pick_scan(g, r, b, mem, u, f);
    if (lane == 0) { n_strat[which] += 1; n_strat[SRW_STRAT_CHAIN] += f; }
    const int32_t next = g.ent[r.off + k].id;
    if (lane == 0) {
      const SWalker nw = shard_advance(wk, step, next, last != 0);
      scratch[ri] = nw;
      if (nw.kind != SK_RET) atomicAdd(&cnt[owner_of_tab(next, io.world, g.owner_tab, g.vmin, g.n_slots)], 1u);
      { const int32_t hm = owner_of_tab(wk.src, io.world, g.owner_tab, g.vmin, g.n_slots);      // every sampled vertex goes home
        if (hm != io.rank) atomicAdd(&cnt[SHARD_MAX_WORLD + hm], 1u); }
      steps += 1; degc += (unsigned long long)r.deg; fb += f;
      if (b.need_member) degp += (unsigned long long)b.prev_deg;
    }
  }
  if (lane == 0)
    for (int i = 0; i < 8; ++i) if (n_strat[i]) atomicAdd(&ctr->strat[i], (unsigned long long)n_strat[i]);
  block_flush_counters(ctr, red, steps, dead, degc, degp, 0, fb);   // contains the __syncthreads() cnt needs
  if (!todo && (int)threadIdx.x < io.world) {
    blk[(int64_t)blockIdx.x * 2 * io.world + threadIdx.x] = cnt[threadIdx.x];
    blk[(int64_t)blockIdx.x * 2 * io.world + io.world + threadIdx.x] = cnt[SHARD_MAX_WORLD + threadIdx.x];
  }
}

// p = q = 1 on a shard: one record per lane through the precomputed CDF + guide table.
template <bool NT>
__global__ __launch_bounds__(TPB) void k_sh_step_fo(GraphView g, ShardIO io, int32_t first_walk, int32_t step, int32_t last,
                                                    RngSpec rng, SWalker *__restrict__ scratch, uint32_t *__restrict__ blk,
                                                    DevCounters *ctr) {
  __shared__ uint32_t cnt[2 * SHARD_MAX_WORLD], pre[SHARD_MAX_WORLD + 1];
  __shared__ unsigned long long red[6];
  if (threadIdx.x < 2 * SHARD_MAX_WORLD) cnt[threadIdx.x] = 0u;
  if (threadIdx.x < 6) red[threadIdx.x] = 0ull;
  const uint32_t n_in = shard_in_prefix(io, pre);
  unsigned long long steps = 0, dead = 0, reads = 0, fb = 0;
  uint32_t lo, hi;
  shard_slice(n_in, TPB, lo, hi);
  for (uint32_t base = lo; base < hi; base += TPB) {
    const uint32_t ri = base + threadIdx.x;
    int32_t o = -1, hm = -1;
    if (ri < hi) {
      const SWalker wk = shard_in_record(io, pre, ri);
      const Row *rp = row_of(g, wk.curr);
      Row r; r.off = 0; r.deg = 0; r.flags = 0;
      if (rp) r = *rp;
      if (r.deg == 0) {
        if (step > 1) ++dead;
        scratch[ri] = shard_dead(wk);
        hm = owner_of_tab(wk.src, io.world, g.owner_tab, g.vmin, g.n_slots);     // death notice to the home rank
        if (hm == io.rank) hm = -1;                                             // (applied in place by k_sh_bucket)
      } else {
        const uint32_t iter = (uint32_t)(first_walk + wk.lw % io.batch);
        float u = draw_uniform(rng, iter, (uint32_t)rng_source(g, wk.src), (uint32_t)step);
        int32_t next;
        if (r.flags & ROW_IRREGULAR) {
          Bias nb; nb.second_order = false; nb.need_member = false; nb.p = nb.q = 1.0f; nb.prev = 0;
          nb.prev_sids = nullptr; nb.prev_deg = 0; nb.vmin = g.vmin;
          next = g.ent[r.off + lane_pick_sequential(g.ent + r.off, r.deg, nb, u)].id; ++fb;
        } else {
          unsigned rd; int32_t k;
          FoEnt e = fo_pick<NT>(g.fo + r.off, r.deg, u, k, rd); reads += rd;
          next = e.id;
        }
        const SWalker nw = shard_advance(wk, step, next, last != 0);
        scratch[ri] = nw;
        ++steps;
        if (nw.kind != SK_RET) o = owner_of_tab(next, io.world, g.owner_tab, g.vmin, g.n_slots);
        hm = owner_of_tab(wk.src, io.world, g.owner_tab, g.vmin, g.n_slots);
        if (hm == io.rank) hm = -1;
      }
    }
    for (int32_t d = 0; d < io.world; ++d) {               // one LDS atomic per wave, destination and kind
      const unsigned long long m = __ballot(o == d), mh = __ballot(hm == d);
      if (lane_id() == 0) {
        if (m) atomicAdd(&cnt[d], (uint32_t)__popcll(m));
        if (mh) atomicAdd(&cnt[SHARD_MAX_WORLD + d], (uint32_t)__popcll(mh));
      }
    }
  }
  block_flush_counters(ctr, red, steps, dead, 0, 0, reads, fb);
  if ((int)threadIdx.x < io.world) {
    blk[(int64_t)blockIdx.x * 2 * io.world + threadIdx.x] = cnt[threadIdx.x];
    blk[(int64_t)blockIdx.x * 2 * io.world + io.world + threadIdx.x] = cnt[SHARD_MAX_WORLD + threadIdx.x];
  }
}

// p = q = 1 on a shard whose compact records carry links into the owners' tables (srw_shard_rows_*): sampling and
// bucketing in ONE pass.  A walker arrives with the link of the vertex it stands on (no row-table read), picks a 16-byte
// record like k_walk_first_order and leaves with that record's link.  Per tile of TPB * SH_R records: every lane samples
// its SH_R records into registers; the waves count their survivors per destination and their returns per home rank in
// LDS (one LDS atomic per wave and distinct destination); 2 * world threads move the block's counts onto the device-wide
// chunk cursors (one global atomic per tile, destination and kind); the lanes store their records straight into the
// destination chunks.  The last block to finish writes the chunk headers and clears the cursors for the next super-step.
#ifndef SRW_SH_R
#define SRW_SH_R 4
#endif
constexpr int SH_R = SRW_SH_R;      // records per lane and tile
constexpr int SH_CUR_DONE = 2 * SHARD_MAX_WORLD;      // cursors[0 .. 2 * MAX): walkers / returns per destination; [DONE]: finished blocks
template <bool NT>
__global__ __launch_bounds__(TPB) void k_sh_step_cfo(GraphView g, ShardIO io, int32_t first_walk, int32_t step, int32_t last,
                                                     RngSpec rng, uint32_t *__restrict__ cursors, ShardDst dst,
                                                     uint32_t *__restrict__ overflow, DevCounters *ctr) {
  __shared__ uint32_t cnt[2 * SHARD_MAX_WORLD], gbase[2 * SHARD_MAX_WORLD], pre[SHARD_MAX_WORLD + 1];
  __shared__ unsigned long long red[6];
  __shared__ uint32_t is_last;
  const int lane = lane_id();
  if (threadIdx.x < 2 * SHARD_MAX_WORLD) cnt[threadIdx.x] = 0u;
  if (threadIdx.x < 6) red[threadIdx.x] = 0ull;
  const uint32_t n_in = shard_in_prefix(io, pre);          // contains the __syncthreads() cnt / red need
  unsigned long long steps = 0, dead = 0, reads = 0, fb = 0;
  Bias nobias; nobias.second_order = false; nobias.need_member = false; nobias.p = nobias.q = 1.0f;
  nobias.prev = 0; nobias.prev_sids = nullptr; nobias.prev_deg = 0; nobias.vmin = g.vmin;
  uint32_t lo, hi;
  shard_slice(n_in, TPB * SH_R, lo, hi);
  for (uint32_t base = lo; base < hi; base += TPB * SH_R) {
    SWalker nw[SH_R];
    int32_t o[SH_R], hm[SH_R], kind[SH_R];
    uint32_t wpos[SH_R], rpos[SH_R];
#pragma unroll
    for (int r = 0; r < SH_R; ++r) {
      const uint32_t ri = base + (uint32_t)r * TPB + threadIdx.x;
      o[r] = -1; hm[r] = -1; kind[r] = SK_WALKER_RET; wpos[r] = 0; rpos[r] = 0;
      if (ri < hi) {
        const SWalker wk = shard_in_record(io, pre, ri);
        const uint64_t link = (uint64_t)(uint32_t)wk.prev | ((uint64_t)(uint32_t)wk.curr << 32);
        const int64_t off = (int64_t)(link & CFO_NOFF_MASK);
        const int32_t deg = (int32_t)((link >> 40) & 0x7FFFFFu);
        nw[r] = wk;
        if (deg == 0) {                                   // dead end (or a source without neighbors): death notice to the home rank
          if (step > 1) ++dead;
          kind[r] = SK_DEAD;
          hm[r] = owner_of_tab(wk.src, io.world, g.owner_tab, g.vmin, g.n_slots);
          if (hm[r] == io.rank) { hm[r] = -1; io.lens[wk.lw] = step; }
        } else {
          const uint32_t iter = (uint32_t)(first_walk + wk.lw % io.batch);
          CfoEnt e;
          if (!(link >> 63)) {
            const uint32_t m = walk_bits24(rng.seed, iter, (uint32_t)rng_source(g, wk.src), (uint32_t)step);
            unsigned rd;
            e = cfo_pick<NT>(g.cfo + off, deg, m, rd, g.cfo_reload != 0); reads += rd;
          } else {                                        // irregular row: the reference's scan, literally; the links are valid for every row
            const float u = draw_uniform(rng, iter, (uint32_t)rng_source(g, wk.src), (uint32_t)step);
            e = g.cfo[off + lane_pick_sequential(g.ent + off, deg, nobias, u)]; ++fb;
          }
          ++steps;
          const uint64_t nl = e.link & ~(0xFull << 36);
          nw[r].v = e.id; nw[r].prev = (int32_t)(uint32_t)nl; nw[r].curr = (int32_t)(uint32_t)(nl >> 32);   // forwarded: the link of the vertex it moves to
          if (last) kind[r] = SK_RET;
          else o[r] = owner_of_tab(e.id, io.world, g.owner_tab, g.vmin, g.n_slots);
          hm[r] = owner_of_tab(wk.src, io.world, g.owner_tab, g.vmin, g.n_slots);
          if (hm[r] == io.rank) { hm[r] = -1; io.pt[(int64_t)step * io.n_rows + wk.lw] = e.id; }
        }
      }
    }
    // positions inside the block's share of every chunk: wave-aggregated LDS atomics, one per distinct destination
#pragma unroll
    for (int r = 0; r < SH_R; ++r) {
      unsigned long long todo = __ballot(o[r] >= 0);
      while (todo) {
        const int d = __builtin_amdgcn_readlane(o[r], __ffsll((long long)todo) - 1);
        const unsigned long long m = __ballot(o[r] == d);
        uint32_t b0 = 0;
        const int leader = __ffsll((long long)m) - 1;
        if (lane == leader) b0 = atomicAdd(&cnt[d], (uint32_t)__popcll(m));
        b0 = (uint32_t)__builtin_amdgcn_readlane((int)b0, leader);
        if (o[r] == d) wpos[r] = b0 + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        todo &= ~m;
      }
      todo = __ballot(hm[r] >= 0);
      while (todo) {
        const int d = __builtin_amdgcn_readlane(hm[r], __ffsll((long long)todo) - 1);
        const unsigned long long m = __ballot(hm[r] == d);
        uint32_t b0 = 0;
        const int leader = __ffsll((long long)m) - 1;
        if (lane == leader) b0 = atomicAdd(&cnt[SHARD_MAX_WORLD + d], (uint32_t)__popcll(m));
        b0 = (uint32_t)__builtin_amdgcn_readlane((int)b0, leader);
        if (hm[r] == d) rpos[r] = b0 + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        todo &= ~m;
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * io.world) {
      const int d = (int)threadIdx.x < io.world ? (int)threadIdx.x : (int)threadIdx.x - io.world;
      const int idx = (int)threadIdx.x < io.world ? d : SHARD_MAX_WORLD + d;
      const uint32_t c = cnt[idx];
      cnt[idx] = 0u;
      uint32_t gb = 0;
      if (c) {
        gb = atomicAdd(&cursors[idx], c);
        if ((uint64_t)gb + c > (uint64_t)((int)threadIdx.x < io.world ? io.cap_w : io.cap_r)) atomicOr(overflow, 1u);
      }
      gbase[idx] = gb;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SH_R; ++r) {
      if (o[r] >= 0) {
        const uint32_t pos = gbase[o[r]] + wpos[r];
        if (pos < (uint32_t)io.cap_w) reinterpret_cast<WWalker *>(dst.p[o[r]] + 16)[pos] = shard_wire_of(nw[r]);
      }
      if (hm[r] >= 0) {
        const uint32_t pos = gbase[SHARD_MAX_WORLD + hm[r]] + rpos[r];
        if (pos < (uint32_t)io.cap_r) {
          SWalker t = nw[r]; t.kind = kind[r];
          reinterpret_cast<WRet *>(dst.p[hm[r]] + 16 + (int64_t)io.cap_w * SW_BYTES)[pos] = shard_ret_of(t);
        }
      }
    }
  }
  block_flush_counters(ctr, red, steps, dead, 0, 0, reads, fb);
  // the last block: chunk headers from the cursors, cursors cleared for the next super-step
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) is_last = atomicAdd(&cursors[SH_CUR_DONE], 1u) == gridDim.x - 1 ? 1u : 0u;
  __syncthreads();
  if (is_last) {
    __threadfence();
    if ((int)threadIdx.x < 2 * io.world) {
      const bool rets = (int)threadIdx.x >= io.world;
      const int d = rets ? (int)threadIdx.x - io.world : (int)threadIdx.x;
      const uint32_t total = atomicExch(&cursors[rets ? SHARD_MAX_WORLD + d : d], 0u);
      const uint32_t cap = (uint32_t)(rets ? io.cap_r : io.cap_w);
      reinterpret_cast<uint32_t *>(dst.p[d])[rets ? 1 : 0] = total < cap ? total : cap;
      atomicMax(&ctr->why[rets ? 1 : 0], (unsigned long long)total);      // the fullest chunk of the batch (run_shard_finish, SRW_TIMING)
    }
    if (threadIdx.x == 0) cursors[SH_CUR_DONE] = 0u;
  }
}

// blk[b][col] (counts) -> blk[b][col] (write cursor of block b inside chunk col's record array); the chunk headers get
// the totals (clamped to the capacity, overflow flagged).  One block; wave w handles columns w, w + nwaves, ...
__global__ void k_sh_offsets(uint32_t *__restrict__ blk, int32_t n_blocks, ShardIO io, ShardDst dst, uint32_t *overflow) {
  const int lane = lane_id(), wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int per = (n_blocks + 63) / 64, cols = 2 * io.world;
  for (int col = wv; col < cols; col += nw) {
    unsigned long long loc = 0;
    for (int i = 0; i < per; ++i) { const int b = lane * per + i; if (b < n_blocks) loc += blk[(int64_t)b * cols + col]; }
    unsigned long long incl = loc;
    for (int o = 1; o < 64; o <<= 1) { unsigned long long t = __shfl_up(incl, o); if (lane >= o) incl += t; }
    unsigned long long run = incl - loc;
    for (int i = 0; i < per; ++i) {
      const int b = lane * per + i;
      if (b < n_blocks) { const uint32_t c = blk[(int64_t)b * cols + col]; blk[(int64_t)b * cols + col] = (uint32_t)run; run += c; }
    }
    const unsigned long long total = (unsigned long long)__shfl((long long)incl, 63);
    if (lane == 0) {
      const bool rets = col >= io.world;
      const int d = rets ? col - io.world : col;
      const uint32_t cap = (uint32_t)(rets ? io.cap_r : io.cap_w);
      uint32_t *h = reinterpret_cast<uint32_t *>(dst.p[d]);
      h[rets ? 1 : 0] = (uint32_t)(total < cap ? total : cap);
      if (total > cap) atomicOr(overflow, 1u);
    }
  }
}

__global__ __launch_bounds__(TPB) void k_sh_bucket(GraphView g, ShardIO io, int32_t unit, int32_t step,
                                                   const SWalker *__restrict__ recs, const uint32_t *__restrict__ blk, ShardDst dst) {
  __shared__ uint32_t cur[2 * SHARD_MAX_WORLD], pre[SHARD_MAX_WORLD + 1];
  const uint32_t n_in = shard_in_prefix(io, pre);
  if ((int)threadIdx.x < io.world) {
    cur[threadIdx.x] = blk[(int64_t)blockIdx.x * 2 * io.world + threadIdx.x];
    cur[SHARD_MAX_WORLD + threadIdx.x] = blk[(int64_t)blockIdx.x * 2 * io.world + io.world + threadIdx.x];
  }
  __syncthreads();
  const int lane = lane_id();
  uint32_t lo, hi;
  shard_slice(n_in, (uint32_t)unit, lo, hi);
  for (uint32_t base = lo; base < hi; base += TPB) {
    const uint32_t i = base + threadIdx.x;
    SWalker w; w.lw = 0; w.src = 0; w.prev = 0; w.curr = 0; w.v = 0; w.kind = SK_RET; w.pad0 = w.pad1 = 0;
    int32_t o = -1, hm = -1;
    if (i < hi) {
      w = recs[i];
      if (w.kind == SK_WALKER_RET) o = owner_of_tab(w.curr, io.world, g.owner_tab, g.vmin, g.n_slots);
      hm = owner_of_tab(w.src, io.world, g.owner_tab, g.vmin, g.n_slots);
      if (hm == io.rank) { hm = -1; shard_return_home(io, w, step); }
    }
    for (int32_t d = 0; d < io.world; ++d) {
      const unsigned long long m = __ballot(o == d);
      if (m) {
        uint32_t b0 = 0;
        const int leader = __ffsll((long long)m) - 1;
        if (lane == leader) b0 = atomicAdd(&cur[d], (uint32_t)__popcll(m));
        b0 = (uint32_t)__builtin_amdgcn_readlane((int)b0, leader);
        const uint32_t pos = b0 + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (o == d && pos < (uint32_t)io.cap_w) reinterpret_cast<WWalker *>(dst.p[d] + 16)[pos] = shard_wire_of(w);
      }
      const unsigned long long mh = __ballot(hm == d);
      if (mh) {
        uint32_t b0 = 0;
        const int leader = __ffsll((long long)mh) - 1;
        if (lane == leader) b0 = atomicAdd(&cur[SHARD_MAX_WORLD + d], (uint32_t)__popcll(mh));
        b0 = (uint32_t)__builtin_amdgcn_readlane((int)b0, leader);
        const uint32_t pos = b0 + (uint32_t)__popcll(mh & ((1ull << lane) - 1ull));
        if (hm == d && pos < (uint32_t)io.cap_r)
          reinterpret_cast<WRet *>(dst.p[d] + 16 + (int64_t)io.cap_w * SW_BYTES)[pos] = shard_ret_of(w);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// q != 1 on a shard that holds the per-edge tables of the pairs into its own rows (edge_tables.hip:prepare_shard_tables):
// the lean table step of k_walk_tables, one super-step at a time.  One wave per incoming walker, persistent waves taking
// groups of records from a cursor (a step costs anything from one row of registers to a located chunk of a hub row).  The
// step's first round trip issues together: the row of curr (local), the membership row of prev (replicated) and the pair
// hash probe that yields the table word eb_off[e] would hold on a whole-graph handle.  Steps without a table (uncertified
// rows, test configurations) go to the todo list: k_sh_step redoes exactly those with the on-the-fly samplers.  The sampled
// records land in `scratch` in input order; k_sh_scatter buckets them.
// records per cursor grab (a single counter word saturates at ~88 atomics/us).  With the BATCH prologue of k_sh_step_tab a grab is also
// what one Philox evaluation / one round of record, row and pair-hash reads serves: 8 -> 1 221 ms, 16 -> 676, 32 -> 608, 64 -> 606 ms per
// iteration at config 3's shape, 3 809 / 3 756 / 3 741 ms at config 5's (profiles/r04_sharded_batch.md); the kernel takes fewer per grab
// when a super-step has fewer than 4 grabs per wave (small shards: the waves would not share the work evenly).
constexpr int SH_GRAB = 32;
// (arguments as one struct, read again from the kernarg segment where a record needs them: k_walk_tables, device_common.h:fresh_args)
struct ShTabArgs {
  GraphView g; ShardIO io; int32_t first_walk, step, last; RngSpec rng; float p, q; SWalker *scratch;
  unsigned long long *cursor; uint32_t *todo; DevCounters *ctr; int32_t grab_n; ChainRec *chain;
};
#define SH_TAB_ARGS() fresh_args<ShTabArgs>()
// BATCH (round 4, SRW_SH_BATCH=0 for the A / B): what a record needs before its first table read — the record itself, its
// Philox draw and the pair-hash probe — is fetched and computed for the WHOLE grab at once, lane l for record r0 + l (one Philox
// evaluation and one probe chain per 16 records instead of 16 wave-wide ones; the record's step then starts at the row reads),
// and every pick goes back through SGPRs (uni) so that the record loop is uniform in the compiler's eyes, as in k_walk_tables.
// BATCH == 2: also the row of curr and the membership row of prev per lane, and the sampled records collected per lane
// (v_writelane) and stored once per grab, coalesced.
#ifndef SRW_SH_LEAN_WAVES                 // (waves per SIMD of the sharded table step: the grab's per-lane state costs 36 B of scratch at 8)
#define SRW_SH_LEAN_WAVES SRW_LEAN_WAVES
#endif
#ifndef SRW_SH_LEAN_WAVES_BF
#define SRW_SH_LEAN_WAVES_BF SRW_LEAN_WAVES_BF
#endif
template <bool BF, int BATCH>
__global__ __launch_bounds__(TPB, BF ? SRW_SH_LEAN_WAVES_BF : SRW_SH_LEAN_WAVES) void k_sh_step_tab(ShTabArgs a0) {
  __shared__ __attribute__((aligned(16))) uint32_t stage_all[TPB / 64][1024];
  __shared__ uint32_t pre[SHARD_MAX_WORLD + 1];
  const int lane = lane_id();
  uint32_t *stage = stage_all[threadIdx.x >> 6];
  const uint32_t n_in = shard_in_prefix(a0.io, pre);
  Member mem; mem.mode = 0; mem.bm = stage; mem.seg_base = 0;
  const int32_t step = a0.step;
  const uint32_t n_waves4 = gridDim.x * (uint32_t)(TPB / 64) * 4u;
  const int32_t grab_n = (int32_t)uni(n_in / n_waves4 >= (uint32_t)a0.grab_n ? (uint32_t)a0.grab_n : (n_in / n_waves4 ? n_in / n_waves4 : 1u));
  const bool second = step > 1;
  unsigned long long srch = 0;
  uint32_t steps = 0, fb = 0, dead = 0, fast = 0, n_tab = 0, n_mask = 0, n_first = 0, n_todo = 0;
  while (true) {
    unsigned long long grab = 0;
    if (lane == 0) grab = atomicAdd(SH_TAB_ARGS().cursor, (unsigned long long)grab_n);
    const uint32_t r0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(grab > 0xFFFFFFFFull ? 0xFFFFFFFFull : grab));
    if (r0 >= n_in) break;
    const uint32_t r1 = r0 + (uint32_t)grab_n < n_in ? r0 + (uint32_t)grab_n : n_in;
    // (BATCH) lane l: record r0 + l, its draw, the table word of its pair (b_eo: bit 0 of b_found = the pair has one)
    SWalker bw; bw.lw = 0; bw.src = 0; bw.prev = 0; bw.curr = 0;
    float bu = 0.0f; uint32_t b_eo = EB_NONE, b_found = 0u;
    Row b_r, b_mr; b_r.off = 0; b_r.deg = 0; b_r.flags = 0; b_mr = b_r;
    int32_t b_next = 0, b_stat = 0;                   // (BATCH == 2) per lane: the sampled vertex, 1 = advance / 2 = dead / 0 = not this kernel's
    if constexpr (BATCH != 0) {
      const ShTabArgs ab = SH_TAB_ARGS();
      const GraphView &g = ab.g;
      const uint32_t rl = r0 + (uint32_t)lane < r1 ? r0 + (uint32_t)lane : r1 - 1u;      // (grab_n <= 64: run_shard_superstep)
      bw = shard_in_record(ab.io, pre, rl);
      const uint32_t iter = (uint32_t)(ab.first_walk + bw.lw % ab.io.batch);
      bu = draw_uniform(ab.rng, iter, (uint32_t)rng_source(g, bw.src), (uint32_t)step);
      const int64_t cslot = (int64_t)bw.curr - g.vmin, pslot = (int64_t)bw.prev - g.vmin;
      if (second && cslot >= 0 && cslot < g.n_slots && pslot >= 0 && pslot < g.n_slots) {
        uint32_t pad;
        if constexpr (BATCH == 2) b_mr = g.mrows[pslot];
        b_found = pair_lookup_lane(g.ph, g.ph_buckets, (uint32_t)pslot, (uint32_t)cslot, b_eo, pad) ? 1u : 0u;
      }
      if constexpr (BATCH == 2) { if (cslot >= 0 && cslot < g.n_slots) b_r = g.rows[cslot]; }
    }
    for (uint32_t ri = r0; ri < r1; ++ri) {
      const ShTabArgs ar = SH_TAB_ARGS();             // (what the top of a record needs; the samplers read the graph again where they start)
      const GraphView &g = ar.g;
      SWalker wk;
      if constexpr (BATCH != 0) {
        const int j = (int)(ri - r0);
        wk.lw = __builtin_amdgcn_readlane(bw.lw, j); wk.src = __builtin_amdgcn_readlane(bw.src, j);
        wk.prev = __builtin_amdgcn_readlane(bw.prev, j); wk.curr = __builtin_amdgcn_readlane(bw.curr, j);
        wk.v = 0; wk.kind = 0; wk.pad0 = 0; wk.pad1 = 0;
      } else {
        wk = shard_in_record(ar.io, pre, ri);
        wk.lw = __builtin_amdgcn_readfirstlane(wk.lw); wk.src = __builtin_amdgcn_readfirstlane(wk.src);
        wk.prev = __builtin_amdgcn_readfirstlane(wk.prev); wk.curr = __builtin_amdgcn_readfirstlane(wk.curr);
      }
      const int64_t cslot = (int64_t)wk.curr - g.vmin, pslot = (int64_t)wk.prev - g.vmin;
      const bool in_range = cslot >= 0 && cslot < g.n_slots;
      Row r, mr;
      uint32_t eo = EB_NONE; bool found = false;
      if constexpr (BATCH == 2) {                        // (zero rows where a slot is out of range: the prologue left them so)
        const int j = (int)(ri - r0);
        r = lane_row(b_r, j); mr = lane_row(b_mr, j);
        eo = (uint32_t)__builtin_amdgcn_readlane((int)b_eo, j); found = __builtin_amdgcn_readlane((int)b_found, j) != 0;
      } else {
        r = g.rows[in_range ? cslot : 0];
        mr.off = 0; mr.deg = 0; mr.flags = 0;
        if (second && in_range && pslot >= 0 && pslot < g.n_slots) {
          mr = g.mrows[pslot];
          if constexpr (BATCH != 0) {
            const int j = (int)(ri - r0);
            eo = (uint32_t)__builtin_amdgcn_readlane((int)b_eo, j); found = __builtin_amdgcn_readlane((int)b_found, j) != 0;
          } else found = pair_lookup_wave(g.ph, g.ph_buckets, (uint32_t)pslot, (uint32_t)cslot, eo);
          mr = uniform_row(mr);
        }
        r = uniform_row(r);
        if (!in_range) { r.off = 0; r.deg = 0; r.flags = 0; }
      }
      if (r.deg == 0) {                                  // dead end (or a source without neighbors): tell the home rank the length
        if constexpr (BATCH == 2) write_lane(b_stat, 2, (int)(ri - r0));
        else if (lane == 0) ar.scratch[ri] = shard_dead(wk);
        dead += second ? 1u : 0u;
        continue;
      }
      float u;
      if constexpr (BATCH != 0) u = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(bu), (int)(ri - r0)));
      else {
        const uint32_t iter = (uint32_t)(ar.first_walk + wk.lw % ar.io.batch);
        u = draw_uniform(ar.rng, iter, (uint32_t)__builtin_amdgcn_readfirstlane(rng_source(g, wk.src)), (uint32_t)step);
      }
      unsigned f = 0, sv = 0;
      int32_t k, next = 0;
      // CHAIN = false: a draw within rounding distance of a CDF boundary is not decided here.  On a table step the record
      // goes to the chain list with the reference's sum S (k_chain_*: the quotients of the whole row computed by the whole
      // GPU, then one sequential pass over them) — one wave running the chain over a hub row alone was the tail of every
      // other super-step; everywhere else (first steps, rows below 256 candidates) the general step takes the record.
      bool to_chain = false; double S_tie = 0.0;
      if (!second) {
        k = wave_pick_first<false>(fresh_graph(), r, u, f, next);
        if constexpr (BATCH != 0) k = uni(k);
        n_first += k >= 0 ? 1u : 0u;
      } else {
        Bias b;
        b.p = ar.p; b.q = ar.q; b.prev = wk.prev; b.second_order = true; b.need_member = true; b.vmin = g.vmin;
        b.prev_sids = g.msids + mr.off; b.prev_deg = mr.deg; b.prev_hub = mr.flags >> ROW_HUB_SHIFT;
        if (r.deg <= g.eb_mask_max && found) {
          k = wave_pick_masked<false>(fresh_graph(), r, b, eo, r.deg > 32 ? g.em_bits + (size_t)eo * 4 : nullptr, u, f, next);
          if constexpr (BATCH != 0) k = uni(k);
          if (k >= 0) { n_mask += 1; srch += 8ull * (unsigned long long)r.deg + 4ull * (unsigned long long)((r.deg + 31) >> 5); }
        } else if (r.deg > g.eb_mask_max && found && (r.flags & ROW_PQ_OK)) {
          k = wave_pick_edge_table<BF, false>(fresh_graph(), r, b, g.eb_bins + (size_t)eo * 8, u, f, sv, mem, next, stage, &S_tie);
          if constexpr (BATCH != 0) k = uni(k);
          if (k >= 0) { n_tab += 1; srch += 8ull * EB_BINS; fast += sv; }
          to_chain = k == CHAIN_NEEDED;
        } else k = -1;
      }
      if (k < 0) {
        const ShTabArgs at = SH_TAB_ARGS();
        unsigned long long *cursor = at.cursor; ChainRec *chain = at.chain; uint32_t *todo = at.todo;
        if (lane == 0) {
          unsigned long long ci = to_chain ? atomicAdd(cursor + 2, 1ull) : (unsigned long long)CHAIN_CAP;
          if (ci < (unsigned long long)CHAIN_CAP) { ChainRec cr; cr.ri = ri; cr.pad = 0u; cr.S = S_tie; chain[ci] = cr; }
          else todo[atomicAdd(cursor + 1, 1ull)] = ri;    // no table for this pair / a full chain list: the general step takes the record
        }
        n_todo += 1;
        continue;
      }
      next = __builtin_amdgcn_readfirstlane(next);
      fb += f; steps += 1;
      if constexpr (BATCH == 2) {
        write_lane(b_next, next, (int)(ri - r0)); write_lane(b_stat, 1, (int)(ri - r0));
      } else if (lane == 0) { const ShTabArgs ao = SH_TAB_ARGS(); ao.scratch[ri] = shard_advance(wk, step, next, ao.last != 0); }
    }
    if constexpr (BATCH == 2) {                          // the grab's sampled records, one per lane
      const ShTabArgs ao = SH_TAB_ARGS();
      if (r0 + (uint32_t)lane < r1 && b_stat != 0)
        ao.scratch[r0 + (uint32_t)lane] = b_stat == 1 ? shard_advance(bw, step, b_next, ao.last != 0) : shard_dead(bw);
    }
  }
  if (lane == 0) {
    DevCounters *ctr = SH_TAB_ARGS().ctr;
    srch += mem.res_bytes;
    if (steps) atomicAdd(&ctr->steps, (unsigned long long)steps);
    if (dead) atomicAdd(&ctr->dead_ends, (unsigned long long)dead);
    if (fb) { atomicAdd(&ctr->fallbacks, (unsigned long long)fb); atomicAdd(&ctr->strat[SRW_STRAT_CHAIN], (unsigned long long)fb); }
    if (fast) atomicAdd(&ctr->ent_reads, (unsigned long long)fast);
    if (srch) atomicAdd(&ctr->trials, srch);
    if (n_tab) atomicAdd(&ctr->strat[SRW_STRAT_EDGE_TABLE], (unsigned long long)n_tab);
    if (n_mask) atomicAdd(&ctr->strat[SRW_STRAT_EDGE_MASK], (unsigned long long)n_mask);
    if (n_first) atomicAdd(&ctr->strat[SRW_STRAT_SCAN], (unsigned long long)n_first);
    if (n_todo) atomicAdd(&ctr->strat[SRW_STAT_HANDED_OVER], (unsigned long long)n_todo);
  }
}

// p != 1, q == 1 on a shard: one record per LANE (k_walk_q1's step, one super-step at a time; round 2 ran this case one wave
// per record through k_sh_step).  Per record: the row of curr (local), the Philox draw, and — second-order steps — the pair's
// return-edge record from the shard's hash (edge_tables.hip:build_shard_rev_hash) + q1_pick over the local compact records and
// exact prefix sums.  An irregular row or a draw within rounding distance of a CDF boundary puts the record on the todo list
// (k_sh_step redoes exactly those); k_sh_scatter buckets the scratch records.
#ifndef SRW_SHQ1_WAVES
#define SRW_SHQ1_WAVES 1          // (minimum waves per SIMD asked of the compiler: 1 = whatever the kernel needs — 86 VGPRs, 5 waves)
#endif
template <bool NT>
__global__ __launch_bounds__(TPB, SRW_SHQ1_WAVES) void k_sh_step_q1(GraphView g, ShardIO io, int32_t first_walk, int32_t step, int32_t last, RngSpec rng, float p,
                                                    SWalker *__restrict__ scratch, unsigned long long *cursor, uint32_t *__restrict__ todo,
                                                    ChainRec *__restrict__ chain, DevCounters *ctr, uint32_t max_ret, uint32_t *__restrict__ many) {
  __shared__ uint32_t pre[SHARD_MAX_WORLD + 1];
  const uint32_t n_in = shard_in_prefix(io, pre);
  unsigned long long steps = 0, dead = 0, reads = 0, n_todo = 0;
  uint32_t lo, hi;
  shard_slice(n_in, TPB, lo, hi);
  for (uint32_t base = lo; base < hi; base += TPB) {
    const uint32_t ri = base + threadIdx.x;
    if (ri >= hi) continue;
    const SWalker wk = shard_in_record(io, pre, ri);
    const Row *rp = row_of(g, wk.curr);
    Row r; r.off = 0; r.deg = 0; r.flags = 0;
    if (rp) r = *rp;
    if (r.deg == 0) { if (step > 1) ++dead; scratch[ri] = shard_dead(wk); continue; }
    bool handed = (r.flags & ROW_IRREGULAR) != 0;
    CfoEnt e; int32_t k = -1;
    if (!handed) {
      const uint32_t iter = (uint32_t)(first_walk + wk.lw % io.batch);
      const uint32_t m = walk_bits24(rng.seed, iter, (uint32_t)rng_source(g, wk.src), (uint32_t)step);
      const CfoEnt *crow = g.cfo + r.off;
      if (step == 1) { unsigned rd; e = cfo_pick<NT>(crow, r.deg, m, rd, k, g.cfo_reload != 0); reads += rd; }
      else {
        uint32_t rv = REV_NONE, pos0 = 0u;
        float w0 = 0.0f;
        if (pair_lookup_lane(g.rh, g.rh_buckets, (uint32_t)((int64_t)wk.prev - g.vmin), (uint32_t)((int64_t)wk.curr - g.vmin), rv, pos0))
          w0 = g.ent[r.off + pos0].w;
        else rv = REV_NONE;
        // many parallel return edges (hub <-> hub multi-edges, a hub's self-loops): every prefix value walks the whole run in ONE
        // lane, and a super-step ends with its slowest lane (RMAT-24: 450 ms per iteration, 140 without them) — one wave per
        // such record instead (k_sh_step_q1w)
        if (rv != REV_NONE && (rv >> 24) > max_ret) { many[atomicAdd(cursor + 3, 1ull)] = ri; continue; }
        double S_tie = 0.0;
        const int why = q1_pick<NT>(g, r, crow, rv, (int32_t)pos0, w0, wk.prev, m, p, e, k, reads, &S_tie);
        if (why == 2) {       // a tie: the exact chain, its quotients computed by the whole GPU (k_chain_d)
          const unsigned long long ci = atomicAdd(cursor + 2, 1ull);
          if (ci < (unsigned long long)CHAIN_CAP) { ChainRec cr; cr.ri = ri; cr.pad = 0u; cr.S = S_tie; chain[ci] = cr; continue; }
        }
        handed = why != 0;
      }
    }
    if (handed) { todo[atomicAdd(cursor + 1, 1ull)] = ri; ++n_todo; continue; }
    scratch[ri] = shard_advance(wk, step, e.id, last != 0);
    ++steps;
  }
  flush_counters(ctr, steps, dead, 0, 0, reads, 0);
  const unsigned long long tot = wave_sum_u64(steps);
  if (lane_id() == 0 && tot) atomicAdd(&ctr->strat[SRW_STRAT_Q1_LANE], tot);
  const unsigned long long nt = wave_sum_u64(n_todo);
  if (lane_id() == 0 && nt) atomicAdd(&ctr->strat[SRW_STAT_HANDED_OVER], nt);
}

// The records of k_sh_step_q1's "many return edges" list, one wave each (wave_pick_returns): picked -> scratch, a tie -> the chain
// list, a row without usable prefix sums -> the general step's todo list.
__global__ __launch_bounds__(TPB) void k_sh_step_q1w(GraphView g, ShardIO io, int32_t first_walk, int32_t step, int32_t last, RngSpec rng, float p,
                                                     SWalker *__restrict__ scratch, unsigned long long *cursor, const uint32_t *__restrict__ many,
                                                     uint32_t *__restrict__ todo, ChainRec *__restrict__ chain, DevCounters *ctr) {
  __shared__ uint32_t pre[SHARD_MAX_WORLD + 1];
  shard_in_prefix(io, pre);
  const int lane = lane_id();
  const uint32_t n = (uint32_t)cursor[3];
  unsigned long long steps = 0, n_todo = 0;
  for (uint32_t ti = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6); ti < n; ti += gridDim.x * (TPB / 64)) {
    const uint32_t ri = many[ti];
    const SWalker wk = shard_record_uniform(io, pre, ri);
    const Row r = uniform_row(*row_of(g, wk.curr));        // (listed: the row exists and is regular)
    const uint32_t xprev = (uint32_t)((int64_t)wk.prev - g.vmin);
    uint32_t rv = 0u;
    int32_t nr = 0; int64_t so = r.off;
    if (pair_lookup_wave(g.rh, g.rh_buckets, xprev, (uint32_t)((int64_t)wk.curr - g.vmin), rv)) {
      so = r.off + (int64_t)(rv & 0xFFFFFFu); nr = (int32_t)(rv >> 24);
      if (nr >= 255) {                                     // the count saturated: the run of prev in the sorted row
        nr = 0;
        for (int64_t c = so;; c += 64) {
          const unsigned long long m = __ballot(c + lane < r.off + r.deg && g.sids[c + lane] == xprev);
          nr += __popcll(m);
          if (m != ~0ull) break;
        }
      }
    }
    Bias b = make_bias(g, p, 1.0f, wk.prev, true);
    const uint32_t iter = (uint32_t)(first_walk + wk.lw % io.batch);
    const float u = draw_uniform(rng, iter, (uint32_t)__builtin_amdgcn_readfirstlane(rng_source(g, wk.src)), (uint32_t)step);
    unsigned f = 0; double S_tie = 0.0;
    const int32_t k = wave_pick_returns<false>(g, r, b, so, nr, u, f, &S_tie);
    if (k == CHAIN_NEEDED) {
      unsigned long long ci = CHAIN_CAP;
      if (lane == 0) ci = atomicAdd(cursor + 2, 1ull);
      ci = (unsigned long long)__builtin_amdgcn_readfirstlane((int)(ci < (unsigned long long)CHAIN_CAP ? ci : CHAIN_CAP));
      if (ci < (unsigned long long)CHAIN_CAP) { if (lane == 0) { ChainRec cr; cr.ri = ri; cr.pad = 0u; cr.S = S_tie; chain[ci] = cr; } continue; }
    }
    if (k < 0) { if (lane == 0) { todo[atomicAdd(cursor + 1, 1ull)] = ri; ++n_todo; } continue; }
    if (lane == 0) { scratch[ri] = shard_advance(wk, step, g.ent[r.off + k].id, last != 0); ++steps; }
  }
  if (lane == 0 && steps) { atomicAdd(&ctr->steps, steps); atomicAdd(&ctr->strat[SRW_STRAT_PREFIX], steps); }
  if (lane == 0 && n_todo) atomicAdd(&ctr->strat[SRW_STAT_HANDED_OVER], n_todo);
}

// Buckets a super-step's sampled records (scratch, input order) into the destination chunks in ONE pass, like the second
// half of k_sh_step_cfo: per tile of TPB * SH_R records the waves count survivors per destination and returns per home rank
// in LDS, 2 * world threads move the block's counts onto the device-wide chunk cursors, the lanes store straight into the
// chunks; the last block writes the chunk headers and clears the cursors.  Replaces k_sh_offsets + k_sh_bucket (and the
// per-block count matrix) for the table steps, whose records are not sampled by fixed slices.
__global__ __launch_bounds__(TPB) void k_sh_scatter(GraphView g, ShardIO io, int32_t step, const SWalker *__restrict__ recs,
                                                    uint32_t *__restrict__ cursors, ShardDst dst, uint32_t *__restrict__ overflow, DevCounters *ctr) {
  __shared__ uint32_t cnt[2 * SHARD_MAX_WORLD], gbase[2 * SHARD_MAX_WORLD], pre[SHARD_MAX_WORLD + 1];
  __shared__ uint32_t is_last;
  const int lane = lane_id();
  if (threadIdx.x < 2 * SHARD_MAX_WORLD) cnt[threadIdx.x] = 0u;
  const uint32_t n_in = shard_in_prefix(io, pre);          // contains the __syncthreads() cnt needs
  uint32_t lo, hi;
  shard_slice(n_in, TPB * SH_R, lo, hi);
  for (uint32_t base = lo; base < hi; base += TPB * SH_R) {
    SWalker w[SH_R];
    int32_t o[SH_R], hm[SH_R];
    uint32_t wpos[SH_R], rpos[SH_R];
#pragma unroll
    for (int r = 0; r < SH_R; ++r) {
      const uint32_t ri = base + (uint32_t)r * TPB + threadIdx.x;
      o[r] = -1; hm[r] = -1; wpos[r] = 0; rpos[r] = 0;
      w[r].lw = 0; w[r].src = 0; w[r].prev = 0; w[r].curr = 0; w[r].v = 0; w[r].kind = SK_RET; w[r].pad0 = w[r].pad1 = 0;
      if (ri < hi) {
        w[r] = recs[ri];
        if (w[r].kind == SK_WALKER_RET) o[r] = owner_of_tab(w[r].curr, io.world, g.owner_tab, g.vmin, g.n_slots);
        hm[r] = owner_of_tab(w[r].src, io.world, g.owner_tab, g.vmin, g.n_slots);
        if (hm[r] == io.rank) { hm[r] = -1; shard_return_home(io, w[r], step); }
      }
    }
#pragma unroll
    for (int r = 0; r < SH_R; ++r) {
      unsigned long long todo = __ballot(o[r] >= 0);
      while (todo) {
        const int d = __builtin_amdgcn_readlane(o[r], __ffsll((long long)todo) - 1);
        const unsigned long long m = __ballot(o[r] == d);
        uint32_t b0 = 0;
        const int leader = __ffsll((long long)m) - 1;
        if (lane == leader) b0 = atomicAdd(&cnt[d], (uint32_t)__popcll(m));
        b0 = (uint32_t)__builtin_amdgcn_readlane((int)b0, leader);
        if (o[r] == d) wpos[r] = b0 + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        todo &= ~m;
      }
      todo = __ballot(hm[r] >= 0);
      while (todo) {
        const int d = __builtin_amdgcn_readlane(hm[r], __ffsll((long long)todo) - 1);
        const unsigned long long m = __ballot(hm[r] == d);
        uint32_t b0 = 0;
        const int leader = __ffsll((long long)m) - 1;
        if (lane == leader) b0 = atomicAdd(&cnt[SHARD_MAX_WORLD + d], (uint32_t)__popcll(m));
        b0 = (uint32_t)__builtin_amdgcn_readlane((int)b0, leader);
        if (hm[r] == d) rpos[r] = b0 + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        todo &= ~m;
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * io.world) {
      const int d = (int)threadIdx.x < io.world ? (int)threadIdx.x : (int)threadIdx.x - io.world;
      const int idx = (int)threadIdx.x < io.world ? d : SHARD_MAX_WORLD + d;
      const uint32_t c = cnt[idx];
      cnt[idx] = 0u;
      uint32_t gb = 0;
      if (c) {
        gb = atomicAdd(&cursors[idx], c);
        if ((uint64_t)gb + c > (uint64_t)((int)threadIdx.x < io.world ? io.cap_w : io.cap_r)) atomicOr(overflow, 1u);
      }
      gbase[idx] = gb;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SH_R; ++r) {
      if (o[r] >= 0) {
        const uint32_t pos = gbase[o[r]] + wpos[r];
        if (pos < (uint32_t)io.cap_w) reinterpret_cast<WWalker *>(dst.p[o[r]] + 16)[pos] = shard_wire_of(w[r]);
      }
      if (hm[r] >= 0) {
        const uint32_t pos = gbase[SHARD_MAX_WORLD + hm[r]] + rpos[r];
        if (pos < (uint32_t)io.cap_r) reinterpret_cast<WRet *>(dst.p[hm[r]] + 16 + (int64_t)io.cap_w * SW_BYTES)[pos] = shard_ret_of(w[r]);
      }
    }
    __syncthreads();                                      // gbase is rewritten by the next tile
  }
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) is_last = atomicAdd(&cursors[SH_CUR_DONE], 1u) == gridDim.x - 1 ? 1u : 0u;
  __syncthreads();
  if (is_last) {
    __threadfence();
    if ((int)threadIdx.x < 2 * io.world) {
      const bool rets = (int)threadIdx.x >= io.world;
      const int d = rets ? (int)threadIdx.x - io.world : (int)threadIdx.x;
      const uint32_t total = atomicExch(&cursors[rets ? SHARD_MAX_WORLD + d : d], 0u);
      const uint32_t cap = (uint32_t)(rets ? io.cap_r : io.cap_w);
      reinterpret_cast<uint32_t *>(dst.p[d])[rets ? 1 : 0] = total < cap ? total : cap;
      atomicMax(&ctr->why[rets ? 1 : 0], (unsigned long long)total);      // the fullest chunk of the batch (run_shard_finish, SRW_TIMING)
    }
    if (threadIdx.x == 0) cursors[SH_CUR_DONE] = 0u;
  }
}
}  // namespace

// ---- host side of one rank (see the kernels above) -------------------------------------------------------------------
void shard_layout(const srw_handle *h, int32_t batch, double slack, srw_shard_layout *out) {
  const int64_t world = h->cfg.world;
  if (batch < 1) throw Error(SRW_ERR_INVALID, "batch must be >= 1");
  if (!(slack >= 1.0)) slack = 1.25;
  // walkers alive at any time <= batch * nVertices, spread over world^2 (sender, receiver) pairs; owner = id mod world
  // (or the recorded partition) mixes hubs and leaves, so the pairs are even up to sampling noise.  A list of start vertices
  // (srw_cluster_set_sources) seeds batch * n walkers instead; its skew over the ranks is the cluster's to put into `slack`.
  const double per_pair = (double)batch * (double)h->shard_walkers_per_iteration() / (double)(world * world);
  const int64_t cap = (int64_t)(per_pair * slack) + 4096;
  if (cap * world >= ((int64_t)1 << 31)) throw Error(SRW_ERR_INVALID, "shard chunks too large (world * capacity must stay below 2^31 records): lower the batch");
  out->cap_walkers = cap; out->cap_rets = cap;
  out->chunk_bytes = 16 + cap * SW_BYTES + cap * PR_BYTES;
}

namespace {
ShardIO make_io(const srw_handle *h, int32_t batch, const srw_shard_layout &lay, const void *d_recv, int32_t *d_lens) {
  ShardIO io;
  io.recv = (const char *)d_recv; io.chunk_bytes = lay.chunk_bytes; io.cap_w = (int32_t)lay.cap_walkers; io.cap_r = (int32_t)lay.cap_rets;
  io.world = h->cfg.world; io.rank = h->cfg.rank; io.batch = batch;
  io.pt = h->shard_pt.p; io.lens = d_lens; io.n_rows = h->shard_rows_per_iteration() * batch;
  return io;
}
void check_shard(const srw_handle *h, int32_t batch, const srw_shard_layout &lay) {
  if (!h->g.loaded) throw Error(SRW_ERR_INVALID, "no graph loaded");
  if (h->cfg.world > SHARD_MAX_WORLD) throw Error(SRW_ERR_INVALID, "world larger than 64 shards");
  if (batch < 1 || lay.cap_walkers < 1 || lay.cap_rets < 1 || lay.chunk_bytes != 16 + lay.cap_walkers * SW_BYTES + lay.cap_rets * PR_BYTES)
    throw Error(SRW_ERR_INVALID, "bad shard layout");
  if ((int64_t)batch * h->shard_rows_per_iteration() >= ((int64_t)1 << 31)) throw Error(SRW_ERR_INVALID, "batch * local vertices must stay below 2^31");
}
}  // namespace

// Seeds this rank's batch * n_local walkers (n_local: its vertices, or its share of the cluster's list of start vertices) into its
// receive buffer, path slot 0 and lens; clears the counters.
// p = q = 1, Philox draws and linked compact records on every shard (srw_shard_rows_commit): the fused kernel
static bool shard_fo_linked(const srw_handle *h, const srw_walk_params &P) {
  return h->g.cfo_linked && P.p == 1.0f && P.q == 1.0f && !(P.flags & (SRW_WALK_FORCE_GENERAL | SRW_WALK_NO_COMPACT)) &&
         P.rng_mode == SRW_RNG_PHILOX;
}

void run_shard_begin(srw_handle *h, const srw_walk_params &P, int32_t batch, const srw_shard_layout &lay, void *d_recv,
                     int32_t *d_paths, int32_t *d_lens, int64_t stride) {
  check_shard(h, batch, lay);
  Graph &g = h->g;
  hipStream_t st = h->stream;
  const int64_t n = h->shard_rows_per_iteration() * batch;
  h->counters.ensure(1);
  h->shard_flag.ensure(1);
  SRW_HIP(hipMemsetAsync(h->counters.p, 0, sizeof(DevCounters), st));
  SRW_HIP(hipMemsetAsync(h->shard_flag.p, 0, 4, st));
  h->shard_pt.ensure((size_t)std::max<int64_t>(n, 1) * (size_t)stride);                // slot-major staging of this batch's paths (k_sh_apply)
  const ShardIO io = make_io(h, batch, lay, d_recv, d_lens);
  const int blocks = (int)std::min<int64_t>(std::max<int64_t>((n + TPB - 1) / TPB, 1), 8192);
  const bool linked = shard_fo_linked(h, P);
  h->shard_cur.ensure((size_t)SH_CUR_DONE + 1);
  SRW_HIP(hipMemsetAsync(h->shard_cur.p, 0, ((size_t)SH_CUR_DONE + 1) * 4, st));
  hipLaunchKernelGGL(k_sh_seed, dim3(blocks), dim3(TPB), 0, st, h->shard_start_verts(), h->shard_rows_per_iteration(), io, (char *)d_recv, h->shard_pt.p, d_lens, stride,
                     linked ? (const Row *)g.rows.p : (const Row *)nullptr, g.vmin, h->shard_flag.p);
  SRW_HIP(hipGetLastError());
}


// One super-step, enqueued on the handle's stream without any host synchronisation: returns of the previous
// super-step applied, every incoming walker sampled once, walkers and path returns bucketed into dst[0 .. world).
void run_shard_superstep(srw_handle *h, const srw_walk_params &P, int32_t batch, int32_t step, const srw_shard_layout &lay,
                         const void *d_recv, void *const *dst, int32_t *d_paths, int32_t *d_lens, int64_t stride) {
  check_shard(h, batch, lay);
  check_params(P);
  if (step < 1 || step > P.walk_length + 1) throw Error(SRW_ERR_INVALID, "step out of range");
  Graph &g = h->g;
  hipStream_t st = h->stream;
  const int32_t world = h->cfg.world;
  const bool first_order = P.p == 1.0f && P.q == 1.0f && !(P.flags & SRW_WALK_FORCE_GENERAL);
  const bool linked = shard_fo_linked(h, P);
  if (world > 1 && P.q != 1.0f && !g.mrows.p)
    throw Error(SRW_ERR_INVALID, "this shard was loaded with SRW_CFG_NO_MEMBERSHIP: it can only run walks with q == 1 "
                                 "(q != 1 needs the neighbor sets of vertices the shard does not own)");
  if (first_order) { build_first_order_tables(h, true); g.use_eb = false; }
  else {
    build_membership(h);
    if (!(P.p == 1.0f && P.q == 1.0f) && !(P.flags & SRW_WALK_NO_PREFIX)) build_pq_tables(h, P.p, P.q);
    else g.has_pq = false;
    // q != 1: the per-edge tables of the pairs into this shard's rows (built at the first super-step of a (p, q))
    if (P.sampler == SRW_SAMPLER_REFERENCE) prepare_shard_tables(h, P); else g.use_eb = false;
  }
  const bool tables = !first_order && g.has_eb && g.use_eb && g.eb_sharded && P.q != 1.0f;
  // p != 1, q == 1: one record per lane when every row holds the prefix-sum certificate and the compact records exist
  bool q1 = false;
  if (!first_order && P.q == 1.0f && P.p != 1.0f && P.rng_mode == SRW_RNG_PHILOX && P.sampler == SRW_SAMPLER_REFERENCE && g.has_pq &&
      g.pq_bad_rows == 0 && ((P.flags >> 12) & 15) == 0 && !(P.flags & (SRW_WALK_NO_PREFIX | SRW_WALK_NO_COMPACT | SRW_WALK_NO_BINNED)) &&
      !getenv("SRW_NO_Q1_KERNEL") && g.n_entries > 0 && build_local_cfo(h)) {
    build_shard_rev_hash(h);
    q1 = true;
  }
  { const char *e = getenv("SRW_DEBUG_CHAIN_DEG"); g.dbg_chain_deg = e && *e ? atoi(e) : 0; }
  const ShardIO io = make_io(h, batch, lay, d_recv, d_lens);
  ShardDst sd;
  for (int d = 0; d < SHARD_MAX_WORLD; ++d) sd.p[d] = d < world ? (char *)dst[d] : nullptr;
  const int n_blocks = h->n_cus * 4;
  h->shard_scratch.ensure((size_t)world * (size_t)lay.cap_walkers * sizeof(SWalker));
  SWalker *scratch = reinterpret_cast<SWalker *>(h->shard_scratch.p);
  h->shard_blk.ensure((size_t)n_blocks * 2 * world);
  h->shard_flag.ensure(1);
  RngSpec rng; rng.mode = P.rng_mode; rng.const_r = P.const_r; rng.seed = P.seed;
  const int32_t last = step == P.walk_length + 1 ? 1 : 0;
  // SRW_SHARD_PROFILE=1 (debug): per-kernel hipEvent times, synchronising after each kernel, printed at the last step
  static const bool prof = getenv("SRW_SHARD_PROFILE") != nullptr;
  double (&acc)[4] = h->shard_prof_acc, (&mx)[4] = h->shard_prof_mx;      // per handle: one host thread per device calls this (cluster.cpp)
  auto timed = [&](int slot, auto &&launch) {
    if (!prof) { launch(); return; }
    SRW_HIP(hipEventRecord(h->ev0, st)); launch(); SRW_HIP(hipEventRecord(h->ev1, st)); SRW_HIP(hipEventSynchronize(h->ev1));
    float ms = 0.f; SRW_HIP(hipEventElapsedTime(&ms, h->ev0, h->ev1)); acc[slot] += ms; mx[slot] = std::max(mx[slot], (double)ms);
    if (slot == 1 && getenv("SRW_SHARD_PROFILE_STEPS")) fprintf(stderr, "[shard step] rank %d step %d: %.2f ms\n", h->cfg.rank, step, ms);
  };
  const int64_t n_rows = h->shard_rows_per_iteration() * batch;
  if (step > 1) timed(0, [&] { hipLaunchKernelGGL(k_sh_apply, dim3(n_blocks), dim3(TPB), 0, st, io, h->shard_pt.p, d_lens, n_rows, step - 1); });
  if (linked) {      // sampling + bucketing in one pass; no scratch, no per-block counts
    h->shard_cur.ensure((size_t)SH_CUR_DONE + 1);
    timed(1, [&] {
      if ((size_t)g.n_entries * sizeof(CfoEnt) > ((size_t)2 << 30))
        hipLaunchKernelGGL(k_sh_step_cfo<true>, dim3(n_blocks), dim3(TPB), 0, st, g.view(), io, P.first_walk, step, last, rng,
                           h->shard_cur.p, sd, h->shard_flag.p, h->counters.p);
      else
        hipLaunchKernelGGL(k_sh_step_cfo<false>, dim3(n_blocks), dim3(TPB), 0, st, g.view(), io, P.first_walk, step, last, rng,
                           h->shard_cur.p, sd, h->shard_flag.p, h->counters.p);
    });
    SRW_HIP(hipGetLastError());
    if (prof && last)
      fprintf(stderr, "[shard profile] rank %d: apply %.1f ms, fused step %.1f ms (cumulative)\n", h->cfg.rank, acc[0], acc[1]);
    return;
  }
  if (q1) {          // per-lane step -> ties through the chain kernels, the rest it hands over through the general step -> one fused bucketing pass
    h->walk_cursor.ensure(4);                       // [1] todo records, [2] chain records, [3] records with many return edges
    const size_t n_rec = (size_t)world * (size_t)lay.cap_walkers;
    h->walk_todo.ensure(2 * n_rec);                 // todo list | many-returns list
    uint32_t *many_list = (uint32_t *)h->walk_todo.p + n_rec;
    h->shard_cur.ensure((size_t)SH_CUR_DONE + 1);
    SRW_HIP(hipMemsetAsync(h->walk_cursor.p, 0, 4 * sizeof(unsigned long long), st));
    const ChainBufs cb = chain_bufs(h);
    ChainRec *chain_list = cb.list;
    const GraphView gv = g.view();
    // a latency-bound kernel of fixed slices: exactly as many blocks as are resident at once
    int (&q1_occ)[2] = h->q1_occ;                     // per handle (one host thread per device)
    const bool ntq = (size_t)g.n_entries * sizeof(CfoEnt) > ((size_t)2 << 30);
    if (!q1_occ[ntq]) {
      int nb = 0;
      if (ntq) SRW_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_sh_step_q1<true>, TPB, 0));
      else SRW_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_sh_step_q1<false>, TPB, 0));
      q1_occ[ntq] = std::max(1, nb);
      if (const char *e = getenv("SRW_SH_Q1_BLOCKS"); e && *e) q1_occ[ntq] = std::max(1, atoi(e));
    }
    const int qb = h->n_cus * q1_occ[ntq];
    const uint32_t q1_max_ret = getenv("SRW_Q1_MAX_RET") ? (uint32_t)atoi(getenv("SRW_Q1_MAX_RET")) : 16u;
    timed(1, [&] {
      if (ntq)
        hipLaunchKernelGGL(k_sh_step_q1<true>, dim3(qb), dim3(TPB), 0, st, gv, io, P.first_walk, step, last, rng, P.p, scratch, h->walk_cursor.p,
                           (uint32_t *)h->walk_todo.p, chain_list, h->counters.p, q1_max_ret, many_list);
      else
        hipLaunchKernelGGL(k_sh_step_q1<false>, dim3(qb), dim3(TPB), 0, st, gv, io, P.first_walk, step, last, rng, P.p, scratch, h->walk_cursor.p,
                           (uint32_t *)h->walk_todo.p, chain_list, h->counters.p, q1_max_ret, many_list);
      hipLaunchKernelGGL(k_sh_step_q1w, dim3(h->n_cus * 8), dim3(TPB), 0, st, gv, io, P.first_walk, step, last, rng, P.p, scratch, h->walk_cursor.p,
                         (const uint32_t *)many_list, (uint32_t *)h->walk_todo.p, chain_list, h->counters.p);
    });
    timed(2, [&] { enqueue_chain(h, cb, gv, io, P, step, last, rng, scratch, (int)SRW_STRAT_Q1_LANE, h->walk_cursor.p, (uint32_t *)h->walk_todo.p); });
    timed(2, [&] {
      hipLaunchKernelGGL(k_sh_step, dim3(n_blocks), dim3(TPB), 0, st, gv, io, P.first_walk, step, last, rng, P.p, P.q, scratch, h->shard_blk.p,
                         h->counters.p, (const uint32_t *)h->walk_todo.p, (const unsigned long long *)(h->walk_cursor.p + 1));
    });
    timed(3, [&] { hipLaunchKernelGGL(k_sh_scatter, dim3(n_blocks), dim3(TPB), 0, st, gv, io, step, scratch, h->shard_cur.p, sd, h->shard_flag.p, h->counters.p); });
    SRW_HIP(hipGetLastError());
    if (prof && last)
      fprintf(stderr, "[shard profile] rank %d: apply %.1f ms, per-lane q = 1 step %.1f ms, general step (handed over) %.1f ms, scatter %.1f ms (cumulative)\n", h->cfg.rank,
              acc[0], acc[1], acc[2], acc[3]);
    return;
  }
  if (tables) {      // lean table step (persistent waves) -> the records without a table through the general step -> one fused bucketing pass
    h->walk_cursor.ensure(4);                       // [0] record cursor, [1] todo records, [2] chain records
    h->walk_todo.ensure((size_t)world * (size_t)lay.cap_walkers);
    h->shard_cur.ensure((size_t)SH_CUR_DONE + 1);
    SRW_HIP(hipMemsetAsync(h->walk_cursor.p, 0, 4 * sizeof(unsigned long long), st));
    const ChainBufs cb = chain_bufs(h);
    ChainRec *chain_list = cb.list;
    const GraphView gv = g.view();
    const char *sge = getenv("SRW_SH_GRAB");
    const int grab_n = std::min(64, sge && *sge ? std::max(1, atoi(sge)) : SH_GRAB);   // (<= 64: one record per lane in the BATCH prologue)
    const char *sbe = getenv("SRW_SH_BATCH");             // (read per super-step: tools/shard_tables_bench.py alternates the variants on one set of tables)
    const int sh_batch = sbe && *sbe ? atoi(sbe) : 2;
    const char *sbl = getenv("SRW_SH_BLOCKS");            // (per super-step, like the two below: tests alternate the variants on one handle)
    const int tb_mult = sbl && *sbl ? std::max(1, atoi(sbl)) : 8;
    const int tb = h->n_cus * tb_mult;
    timed(1, [&] {
      ShTabArgs ta;
      ta.g = gv; ta.io = io; ta.first_walk = P.first_walk; ta.step = step; ta.last = last; ta.rng = rng; ta.p = P.p; ta.q = P.q; ta.scratch = scratch;
      ta.cursor = h->walk_cursor.p; ta.todo = (uint32_t *)h->walk_todo.p; ta.ctr = h->counters.p; ta.grab_n = grab_n; ta.chain = chain_list;
      if (sh_batch == 2) {
        if (gv.bf_off) hipLaunchKernelGGL((k_sh_step_tab<true, 2>), dim3(tb), dim3(TPB), 0, st, ta);
        else hipLaunchKernelGGL((k_sh_step_tab<false, 2>), dim3(tb), dim3(TPB), 0, st, ta);
      } else if (sh_batch == 1) {
        if (gv.bf_off) hipLaunchKernelGGL((k_sh_step_tab<true, 1>), dim3(tb), dim3(TPB), 0, st, ta);
        else hipLaunchKernelGGL((k_sh_step_tab<false, 1>), dim3(tb), dim3(TPB), 0, st, ta);
      } else {
        if (gv.bf_off) hipLaunchKernelGGL((k_sh_step_tab<true, 0>), dim3(tb), dim3(TPB), 0, st, ta);
        else hipLaunchKernelGGL((k_sh_step_tab<false, 0>), dim3(tb), dim3(TPB), 0, st, ta);
      }
    });
    // draws on a CDF boundary of a table step
    timed(2, [&] { enqueue_chain(h, cb, gv, io, P, step, last, rng, scratch, (int)SRW_STRAT_EDGE_TABLE, h->walk_cursor.p, (uint32_t *)h->walk_todo.p); });
    timed(2, [&] {      // (the few records without a table, or whose tie is not a table step's)
      hipLaunchKernelGGL(k_sh_step, dim3(n_blocks), dim3(TPB), 0, st, gv, io, P.first_walk, step, last, rng, P.p, P.q, scratch, h->shard_blk.p,
                         h->counters.p, (const uint32_t *)h->walk_todo.p, (const unsigned long long *)(h->walk_cursor.p + 1));
    });
    timed(3, [&] { hipLaunchKernelGGL(k_sh_scatter, dim3(n_blocks), dim3(TPB), 0, st, gv, io, step, scratch, h->shard_cur.p, sd, h->shard_flag.p, h->counters.p); });
    SRW_HIP(hipGetLastError());
    if (prof && last)
      fprintf(stderr, "[shard profile] rank %d: apply %.1f ms, table step %.1f ms (longest super-step %.1f ms), chain + general step (ties, todo) %.1f ms, scatter %.1f ms (cumulative)\n", h->cfg.rank,
              acc[0], acc[1], mx[1], acc[2], acc[3]);
    return;
  }
  timed(1, [&] {
    if (first_order) {
      // records larger than the caches are read once per fetch: L1-bypassing loads (as k_walk_first_order)
      if ((size_t)g.n_entries * sizeof(FoEnt) > ((size_t)2 << 30))
        hipLaunchKernelGGL(k_sh_step_fo<true>, dim3(n_blocks), dim3(TPB), 0, st, g.view(), io, P.first_walk, step, last, rng,
                           scratch, h->shard_blk.p, h->counters.p);
      else
        hipLaunchKernelGGL(k_sh_step_fo<false>, dim3(n_blocks), dim3(TPB), 0, st, g.view(), io, P.first_walk, step, last, rng,
                           scratch, h->shard_blk.p, h->counters.p);
    } else
      hipLaunchKernelGGL(k_sh_step, dim3(n_blocks), dim3(TPB), 0, st, g.view(), io, P.first_walk, step, last, rng, P.p, P.q,
                         scratch, h->shard_blk.p, h->counters.p, (const uint32_t *)nullptr, (const unsigned long long *)nullptr);
  });
  timed(2, [&] { hipLaunchKernelGGL(k_sh_offsets, dim3(1), dim3(1024), 0, st, h->shard_blk.p, n_blocks, io, sd, h->shard_flag.p); });
  timed(3, [&] {
    hipLaunchKernelGGL(k_sh_bucket, dim3(n_blocks), dim3(TPB), 0, st, g.view(), io, first_order ? TPB : TPB / 64, step,
                       scratch, h->shard_blk.p, sd);
  });
  SRW_HIP(hipGetLastError());
  if (prof && last) {
    fprintf(stderr, "[shard profile] rank %d: apply %.1f ms, step %.1f ms, offsets %.1f ms, bucket %.1f ms (cumulative)\n", h->cfg.rank, acc[0],
            acc[1], acc[2], acc[3]);
  }
}

// After the exchange that follows the last super-step: its path returns.
void run_shard_flush(srw_handle *h, const srw_walk_params &P, int32_t batch, const srw_shard_layout &lay, const void *d_recv,
                     int32_t *d_paths, int32_t *d_lens, int64_t stride) {
  check_shard(h, batch, lay);
  const ShardIO io = make_io(h, batch, lay, d_recv, d_lens);
  const int64_t n_rows = h->shard_rows_per_iteration() * batch;
  hipLaunchKernelGGL(k_sh_apply, dim3(h->n_cus * 4), dim3(TPB), 0, h->stream, io, h->shard_pt.p, d_lens, n_rows, P.walk_length + 1);
  if (n_rows > 0) {      // the staging becomes the caller's [row][L + 2] matrix (-1 beyond each row's length)
    const int64_t tb = std::min<int64_t>((n_rows + 63) / 64, (int64_t)h->n_cus * 16);
    hipLaunchKernelGGL(k_sh_transpose, dim3((unsigned)tb), dim3(TPB), 0, h->stream, (const int32_t *)h->shard_pt.p, (const int32_t *)d_lens, n_rows, stride, d_paths);
  }
  SRW_HIP(hipGetLastError());
  // compacted ids: the home rank's paths are complete now (one flush per begin); they leave with the ids of the input
  if (h->g.compact && n_rows > 0) paths_to_ids(h, d_paths, d_lens, n_rows, stride);
}

// Synchronises the handle's stream; counters accumulated since run_shard_begin and the overflow flag.
void run_shard_finish(srw_handle *h, srw_walk_stats *stats, int32_t *overflow) {
  srw_walk_stats local; srw_walk_stats *s = stats ? stats : &local; memset(s, 0, sizeof(*s));
  uint32_t flag = 0;
  h->shard_flag.ensure(1);
  SRW_HIP(hipMemcpyAsync(&flag, h->shard_flag.p, 4, hipMemcpyDeviceToHost, h->stream));
  read_counters(h, s);                                  // synchronises
  if (getenv("SRW_TIMING")) {
    unsigned long long fill[2] = {0, 0};
    SRW_HIP(hipMemcpy(fill, h->counters.p->why, 16, hipMemcpyDeviceToHost));
    if (fill[0] || fill[1]) fprintf(stderr, "[shard %d/%d] fullest chunk of the batch: %llu walkers, %llu returns%s\n", h->cfg.rank, h->cfg.world, fill[0], fill[1], flag ? " (OVERFLOW)" : "");
  }
  if (overflow) *overflow = (int32_t)flag;
}

}  // namespace srw
