// walk_shared.h — __device__ helpers that more than one family of walk kernels uses (walk_kernels.hip, shard_kernels.hip, chain_kernels.hip).
#pragma once
#include "walk_records.h"

namespace srw {

__device__ inline const Row *row_of(const GraphView &g, int32_t v) {
  int64_t s = (int64_t)v - g.vmin;
  if (s < 0 || s >= g.n_slots) return nullptr;
  return g.rows + s;
}

__device__ inline void flush_counters(DevCounters *ctr, unsigned long long steps, unsigned long long dead,
                                      unsigned long long degc, unsigned long long degp, unsigned long long reads,
                                      unsigned long long fb) {
  steps = wave_sum_u64(steps); dead = wave_sum_u64(dead); degc = wave_sum_u64(degc);
  degp = wave_sum_u64(degp); reads = wave_sum_u64(reads); fb = wave_sum_u64(fb);
  if (lane_id() == 0) {
    if (steps) atomicAdd(&ctr->steps, steps);
    if (dead) atomicAdd(&ctr->dead_ends, dead);
    if (degc) atomicAdd(&ctr->sum_deg_curr, degc);
    if (degp) atomicAdd(&ctr->sum_deg_prev, degp);
    if (reads) atomicAdd(&ctr->ent_reads, reads);
    if (fb) atomicAdd(&ctr->fallbacks, fb);
  }
}

// ---------------------------------------------------------------------------------------------------------
// The second-order step of the q = 1 per-lane kernels (k_walk_q1, k_sh_step_q1): first k that is not a certain miss under the exact
// prefix sums PQ + the return edges' corrections.  rv / rv_pos0 / rv_w0: the pair's return-edge record (RevEnt: count << 24 | index in
// curr's sorted row, input-order position and weight of the first one).  0: picked (k, e = its compact record); 1: non-positive sum,
// 2: a draw within rounding distance of a CDF boundary — the caller hands the walker to the general sampler (or, with the row's
// sum in *S_out, to the chain kernels).
template <bool NT>
__device__ inline int q1_pick(const GraphView &g, const Row &r, const CfoEnt *crow, uint32_t rv, int32_t rv_pos0, float rv_w0, int32_t prev_id,
                              uint32_t m, float p, CfoEnt &e, int32_t &k, unsigned long long &reads, double *S_out = nullptr) {
  const PqRow PQ(g, r.off);
  int32_t rp[REV_MAX_RETURNS]; double rc[REV_MAX_RETURNS];      // return edges: input-order position, correction
  int nr = 0;
  double corr_all = 0.0;
  int64_t so = 0;                                   // first return edge in curr's sorted row
  if (rv != REV_NONE) {
    nr = (int)(rv >> 24);
    so = r.off + (int64_t)(rv & 0xFFFFFFu);
    if (nr >= 255) {                                 // the count saturated (hub <-> hub multi-edges): count the run of prev
      const uint32_t xprev = (uint32_t)((int64_t)prev_id - g.vmin);
      const int64_t row_end = r.off + r.deg;
      while (so + nr < row_end && g.sids[so + nr] == xprev) ++nr;
    }
#pragma unroll
    for (int i = 0; i < REV_MAX_RETURNS; ++i) {
      rp[i] = r.deg; rc[i] = 0.0;
      if (i < nr) {
        float w;
        if (i == 0) { rp[0] = rv_pos0; w = rv_w0; }             // the first return edge travels with rev[e]
        else { rp[i] = (int32_t)g.sperm[so + i]; w = g.sw[so + i]; }
        rc[i] = (double)div_exact(w, p) - (double)w; corr_all += rc[i];
      }
    }
    for (int i = REV_MAX_RETURNS; i < nr; ++i) { const float w = g.sw[so + i]; corr_all += (double)div_exact(w, p) - (double)w; }   // (small graphs: dozens of duplicates between hubs)
  } else {
#pragma unroll
    for (int i = 0; i < REV_MAX_RETURNS; ++i) { rp[i] = r.deg; rc[i] = 0.0; }
  }
  {
    const double S0 = PQ[r.deg - 1], S = S0 + corr_all;
    const double pS = (double)m * 0x1p-24 * S;
    auto corr_upto = [&](int32_t kk) {
      double a = 0.0;
#pragma unroll
      for (int i = 0; i < REV_MAX_RETURNS; ++i) a += (rp[i] <= kk) ? rc[i] : 0.0;       // exact under the certificate
      for (int i = REV_MAX_RETURNS; i < nr; ++i)
        if ((int32_t)g.sperm[so + i] <= kk) { const float w = g.sw[so + i]; a += (double)div_exact(w, p) - (double)w; }
      return a;
    };
    auto numer = [&](int32_t kk) { return PQ[kk] + corr_upto(kk); };
    auto not_miss = [&](int32_t kk, double num) { return !(num * (1.0 + (double)(kk + 8) * 0x1p-51) < pS); };
    // start position: the guide entry of the bucket the target falls into in UNBIASED units (any start is
    // correct, the loops below decide with the exact sums; a good one makes them O(1))
    auto guide_start = [&](double tau, bool &ok) {
      double f = tau / S0;
      f = f < 0.0 ? 0.0 : (f > 0.99999994 ? 0.99999994 : f);
      const uint32_t mm = (uint32_t)(f * 16777216.0);
      const uint32_t j = (uint32_t)(((uint64_t)mm * (uint64_t)(uint32_t)r.deg) >> 24);
      const CfoEnt ge = load_cfo<NT>(crow + j); ++reads;
      const int32_t gd = cfo_delta(ge.cg, ge.link);
      if (gd == CFO_GD_SAT) { ok = false; return 0; }      // no guide for this bucket: bisection below
      const int32_t st = (int32_t)j - gd;
      return st < 0 ? 0 : (st >= r.deg ? r.deg - 1 : st);
    };
    bool ok = S > 0.0 && S0 > 0.0;
    int32_t k0 = 0;
    if (ok) {
      k0 = guide_start(pS, ok);
      const double cb = ok ? corr_upto(k0) : 0.0;
      if (ok && cb != 0.0) {                           // past a return edge: its correction moves the answer
        int32_t first_r = r.deg;
#pragma unroll
        for (int i = 0; i < REV_MAX_RETURNS; ++i) first_r = rp[i] < first_r ? rp[i] : first_r;
        for (int i = REV_MAX_RETURNS; i < nr; ++i) { const int32_t q_ = (int32_t)g.sperm[so + i]; first_r = q_ < first_r ? q_ : first_r; }
        const int32_t k1 = guide_start(pS - cb, ok);
        k0 = k1 < first_r ? first_r : k1;
      }
    }
    const bool usable = S > 0.0 && S0 > 0.0;
    if (!usable) return 1;
    else if (S_out && g.dbg_chain_deg && r.deg >= g.dbg_chain_deg) { *S_out = S; return 2; }
    else {
      // first k that is not a certain miss (A' is non-decreasing, the tolerance grows with k: monotone) — a few
      // steps from the guide's start, else (saturated guide entry, many parallel return edges) by bisection
      int guard = 0;
      double nk = 0.0;
      if (ok) {
        nk = numer(k0);
        bool nm = not_miss(k0, nk);
        while (nm && k0 > 0 && guard < 12) {             // step back while the predecessor is not a certain miss either
          const double np = numer(k0 - 1);
          if (!not_miss(k0 - 1, np)) break;
          --k0; nk = np; ++guard;
        }
        while (!nm && guard < 12) {                      // step forward to the first not-certain-miss
          ++k0; ++guard;
          if (k0 >= r.deg) break;
          nk = numer(k0); nm = not_miss(k0, nk);
        }
        reads += (unsigned)guard + 1u;
      }
      if (!ok || guard >= 12) {
        int32_t lo = 0, hi = r.deg;
        while (lo < hi) {
          const int32_t mid = lo + ((hi - lo) >> 1);
          if (not_miss(mid, numer(mid))) hi = mid; else lo = mid + 1;
          ++reads;
        }
        k0 = lo;
        if (k0 < r.deg) nk = numer(k0);
      }
      if (k0 >= r.deg) { k = 0; e = load_cfo<NT>(crow); ++reads; }                    // no crossing: edges.head (:24)
      else if (nk * (1.0 - (double)(k0 + 8) * 0x1p-51) >= pS) { k = k0; e = load_cfo<NT>(crow + k); ++reads; }   // a certain hit
      else { if (S_out) *S_out = S; return 2; }   // a draw within rounding distance of a boundary: exact chain (S: the reference's sum, exact under the certificate)
    }
  }
  return 0;
}

// ---- a super-step's incoming chunks (described with the k_sh_* kernels in shard_kernels.hip)
__device__ inline const uint32_t *chunk_hdr(const char *base, int64_t cb, int c) { return reinterpret_cast<const uint32_t *>(base + c * cb); }
__device__ inline const WWalker *chunk_walkers(const char *base, int64_t cb, int c) { return reinterpret_cast<const WWalker *>(base + c * cb + 16); }
__device__ inline const WRet *chunk_rets(const char *base, int64_t cb, int32_t cap_w, int c) {
  return reinterpret_cast<const WRet *>(base + c * cb + 16 + (int64_t)cap_w * SW_BYTES);
}

// prefix of the incoming walkers per chunk -> LDS pre[0 .. world]; returns the total
__device__ inline uint32_t shard_in_prefix(const ShardIO &io, uint32_t *pre) {
  if (threadIdx.x == 0) {
    uint32_t acc = 0;
    for (int c = 0; c < io.world; ++c) { pre[c] = acc; acc += min(chunk_hdr(io.recv, io.chunk_bytes, c)[0], (uint32_t)io.cap_w); }
    pre[io.world] = acc;
  }
  __syncthreads();
  return pre[io.world];
}
__device__ inline SWalker shard_in_record(const ShardIO &io, const uint32_t *pre, uint32_t i) {
  int c = 0;
  while (c + 1 < io.world && i >= pre[c + 1]) ++c;
  const WWalker w = chunk_walkers(io.recv, io.chunk_bytes, c)[i - pre[c]];
  SWalker r; r.lw = w.lw; r.src = w.src; r.prev = w.prev; r.curr = w.curr; r.v = 0; r.kind = 0; r.pad0 = 0; r.pad1 = 0;
  return r;
}
__device__ inline SWalker shard_record_uniform(const ShardIO &io, const uint32_t *pre, uint32_t ri) {
  SWalker wk = shard_in_record(io, pre, ri);
  wk.lw = __builtin_amdgcn_readfirstlane(wk.lw); wk.src = __builtin_amdgcn_readfirstlane(wk.src);
  wk.prev = __builtin_amdgcn_readfirstlane(wk.prev); wk.curr = __builtin_amdgcn_readfirstlane(wk.curr);
  return wk;
}

// What happens to a walker that has just sampled `next` (or died): the scratch record the bucketing kernel turns into a
// forwarded walker (unless this was the last step) and the return that carries `next` home.
__device__ inline SWalker shard_advance(const SWalker &wk, int32_t step, int32_t next, bool last) {
  SWalker nw = wk;
  nw.prev = wk.curr; nw.curr = next; nw.v = next;
  nw.kind = last ? SK_RET : SK_WALKER_RET;
  return nw;
}

}  // namespace srw
