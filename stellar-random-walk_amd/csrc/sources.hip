// sources.hip — walks from a caller-supplied list of start vertices (srw_set_sources / srw_set_sources_device).
//
// The walk kernels seed walker wi from verts[wi % n_verts] and key every draw by (seed, iteration, source id, step): nothing in them
// depends on verts being the list of ALL present vertices.  What this file adds is the list itself — the caller's ids, checked
// against the graph and turned into what the kernels expect to find in verts[] (the id, or the slot on a graph whose ids were
// compacted at load) — kept on the handle in the caller's order, duplicates included.  launch_walk reads it through
// srw_handle::start_verts() / walkers_per_iteration().
//
// The vertex-sharded walk (srw_cluster_set_sources) takes the same list: a walker's path lives on owner(source), so every shard is
// handed the whole list, keeps the entries it owns — in list order, with their positions — and seeds those; its path row
// lw = (index in the owned sublist) * batch + iteration leaves for canonical row iteration * n + position (cluster.cpp).
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "engine.h"

namespace srw {
namespace {
constexpr int TPB = 256;
constexpr unsigned long long NO_BAD = ~0ull;

// One lane per list entry.  ids[i] is a vertex id as the input spelled it; out[i] receives the entry of the handle's vertex list
// (verts[n_verts], ascending: ids, or slots when orig_id != nullptr) that stands for it.  An id that is no vertex of the graph
// leaves out[i] = vmin (never read: the call fails) and lowers *bad to (position << 32 | id): the smallest word names the first one.
__global__ __launch_bounds__(TPB) void k_sources_resolve(const int32_t *__restrict__ ids, int64_t n, const int32_t *__restrict__ verts,
                                                         int64_t n_verts, const int32_t *__restrict__ orig_id, int64_t n_slots,
                                                         int32_t vmin, int32_t *__restrict__ out, unsigned long long *bad) {
  const int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x;
  if (i >= n) return;
  const int32_t id = ids[i];
  bool ok = true;
  int32_t v = id;                                      // what the walk kernels know the vertex by
  if (orig_id) {                                       // compacted ids: slot = rank among the sorted distinct input ids
    const int64_t s = lower_bound_i32(orig_id, n_slots, id);
    ok = s < n_slots && orig_id[s] == id;
    v = (int32_t)((int64_t)vmin + s);
  }
  if (ok) {
    const int64_t k = lower_bound_i32(verts, n_verts, v);
    ok = k < n_verts && verts[k] == v;
  }
  out[i] = ok ? v : vmin;
  if (!ok) atomicMin(bad, ((unsigned long long)i << 32) | (uint32_t)id);
}

// The sharded form, one lane per list entry: keep[i] = 1 and out[i] = the verts[] spelling of ids[i] when THIS rank owns the vertex,
// keep[i] = 0 otherwise.  owner() is the shard's own (owner_of_tab over the slot on a graph with compacted ids, like the build), so a
// VCut partition map / the HashPartitioner table are honoured.  verts[n_verts]: this shard's vertices.  An owned id that is no vertex
// lowers *bad; so does an id that has no slot at all — it has no owner either, and is assigned to owner_of(id): exactly one shard
// reports every unknown id, and the smallest word over the shards names the first.
__global__ __launch_bounds__(TPB) void k_shard_sources_resolve(const int32_t *__restrict__ ids, int64_t n, const int32_t *__restrict__ verts,
                                                               int64_t n_verts, const int32_t *__restrict__ orig_id, int64_t n_slots,
                                                               int32_t vmin, int32_t world, int32_t rank, const int32_t *__restrict__ otab,
                                                               int32_t *__restrict__ out, uint8_t *__restrict__ keep, unsigned long long *bad) {
  const int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x;
  if (i >= n) return;
  const int32_t id = ids[i];
  bool ok = true, mine;
  int32_t v = id;
  if (orig_id) {
    const int64_t s = lower_bound_i32(orig_id, n_slots, id);
    ok = s < n_slots && orig_id[s] == id;
    v = (int32_t)((int64_t)vmin + s);
  }
  if (!ok) mine = owner_of(id, world) == rank;
  else {
    mine = owner_of_tab(v, world, otab, vmin, n_slots) == rank;
    if (mine) {
      const int64_t k = lower_bound_i32(verts, n_verts, v);
      ok = k < n_verts && verts[k] == v;
    }
  }
  out[i] = v;
  keep[i] = (mine && ok) ? 1 : 0;
  if (mine && !ok) atomicMin(bad, ((unsigned long long)i << 32) | (uint32_t)id);
}
}  // namespace

unsigned long long shard_resolve_sources(srw_handle *h, const int32_t *h_ids, int64_t n, ShardSources &out) {
  Graph &g = h->g;
  if (!g.loaded) throw Error(SRW_ERR_INVALID, "srw_cluster_set_sources: no graph loaded");
  if (n < 0 || n >= ((int64_t)1 << 31)) throw Error(SRW_ERR_INVALID, "srw_cluster_set_sources: n must be in [0, 2^31)");
  if (n > 0 && !h_ids) throw Error(SRW_ERR_INVALID, "srw_cluster_set_sources: ids is null");
  out.n_list = n; out.n_owned = 0; out.pos_host.clear();
  if (n == 0) return NO_BAD;
  hipStream_t st = h->stream;
  DevBuf<int32_t> all; DevBuf<uint8_t> keep; DevBuf<unsigned long long> cnt; DevBuf<char> temp;
  all.alloc((size_t)n); keep.alloc((size_t)n); cnt.alloc(1);
  h->src_ids.ensure((size_t)n);
  h->src_bad.ensure(1);
  SRW_HIP(hipMemcpyAsync(h->src_ids.p, h_ids, (size_t)n * 4, hipMemcpyHostToDevice, st));
  SRW_HIP(hipMemsetAsync(h->src_bad.p, 0xFF, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_shard_sources_resolve, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, st, (const int32_t *)h->src_ids.p, n,
                     (const int32_t *)g.verts.p, g.n_local_vertices, g.compact ? (const int32_t *)g.orig_id.p : nullptr, g.n_slots, g.vmin,
                     h->cfg.world, h->cfg.rank, (const int32_t *)g.owner_tab.p, all.p, keep.p, h->src_bad.p);
  SRW_HIP(hipGetLastError());
  unsigned long long bad = NO_BAD, n_r = 0;
  SRW_HIP(hipMemcpyAsync(&bad, h->src_bad.p, sizeof(bad), hipMemcpyDeviceToHost, st));
  // the kept entries, stably: their verts[] spelling and their list positions (rocprim::select keeps the input order)
  out.verts.alloc((size_t)n); out.pos.alloc((size_t)n);
  rocprim::counting_iterator<int32_t> iota(0);
  size_t tb = 0, tb2 = 0;
  SRW_HIP(rocprim::select(nullptr, tb, all.p, keep.p, out.verts.p, cnt.p, (size_t)n, st));
  SRW_HIP(rocprim::select(nullptr, tb2, iota, keep.p, out.pos.p, cnt.p, (size_t)n, st));
  tb = tb2 = std::max(tb, tb2);
  temp.alloc(tb);
  SRW_HIP(rocprim::select((void *)temp.p, tb, all.p, keep.p, out.verts.p, cnt.p, (size_t)n, st));
  SRW_HIP(rocprim::select((void *)temp.p, tb2, iota, keep.p, out.pos.p, cnt.p, (size_t)n, st));
  SRW_HIP(hipMemcpyAsync(&n_r, cnt.p, sizeof(n_r), hipMemcpyDeviceToHost, st));
  SRW_HIP(hipStreamSynchronize(st));
  if (bad != NO_BAD) return bad;
  if (n_r > (unsigned long long)n) throw Error(SRW_ERR_HIP, "srw_cluster_set_sources: the owned sublist is longer than the list");
  out.n_owned = (int64_t)n_r;
  out.pos_host.resize((size_t)n_r);
  if (n_r) SRW_HIP(hipMemcpy(out.pos_host.data(), out.pos.p, (size_t)n_r * 4, hipMemcpyDeviceToHost));
  return NO_BAD;
}

void shard_commit_sources(srw_handle *h, ShardSources &&s) {
  h->sh_src_verts = std::move(s.verts); h->sh_src_pos = std::move(s.pos); h->sh_src_pos_host = std::move(s.pos_host);
  h->sh_n_sources = s.n_owned; h->sh_list_len = s.n_list;
}

void shard_clear_sources(srw_handle *h) {
  h->sh_n_sources = -1; h->sh_list_len = -1;
  h->sh_src_verts.release(); h->sh_src_pos.release();
  h->sh_src_pos_host.clear();
}

void set_sources(srw_handle *h, const int32_t *h_ids, const void *d_ids, int64_t n) {
  Graph &g = h->g;
  if (!g.loaded) throw Error(SRW_ERR_INVALID, "srw_set_sources: no graph loaded");
  if (h->cfg.world != 1)
    throw Error(SRW_ERR_INVALID, "srw_set_sources needs a whole-graph handle (world == 1): one shard cannot check or commit a list on its own (srw_cluster_set_sources does it for all of them)");
  if (n < 0 || n >= ((int64_t)1 << 31)) throw Error(SRW_ERR_INVALID, "srw_set_sources: n must be in [0, 2^31)");
  if (n > 0 && !h_ids && !d_ids) throw Error(SRW_ERR_INVALID, "srw_set_sources: ids is null");
  if (n == 0) { h->n_sources = 0; return; }             // a valid list: zero walkers
  hipStream_t st = h->stream;
  DevBuf<int32_t> out;
  out.alloc((size_t)n);
  h->src_ids.ensure((size_t)n);
  h->src_bad.ensure(1);
  SRW_HIP(hipMemcpyAsync(h->src_ids.p, h_ids ? (const void *)h_ids : d_ids, (size_t)n * 4, h_ids ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
  SRW_HIP(hipMemsetAsync(h->src_bad.p, 0xFF, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_sources_resolve, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, st, (const int32_t *)h->src_ids.p, n,
                     (const int32_t *)g.verts.p, g.n_vertices, g.compact ? (const int32_t *)g.orig_id.p : nullptr, g.n_slots, g.vmin, out.p,
                     h->src_bad.p);
  SRW_HIP(hipGetLastError());
  unsigned long long bad = NO_BAD;
  SRW_HIP(hipMemcpyAsync(&bad, h->src_bad.p, sizeof(bad), hipMemcpyDeviceToHost, st));
  SRW_HIP(hipStreamSynchronize(st));
  if (bad != NO_BAD) {
    const int32_t id = (int32_t)(uint32_t)bad;
    throw Error(SRW_ERR_INVALID, "srw_set_sources: id " + std::to_string(id) + " at position " + std::to_string(bad >> 32) +
                                     " is not a vertex of the loaded graph");
  }
  h->src_verts = std::move(out);
  h->n_sources = n;
}

}  // namespace srw
