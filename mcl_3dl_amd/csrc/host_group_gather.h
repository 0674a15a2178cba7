// host_group_gather.h — part of the single translation unit mcl3dl_hip.hip, behind host_group.h: ONE sharded per-particle array
// of floats (the resident states, their odometry noise, their weights) brought into particle order on every rank. ROUTE_DIRECT:
// the rank's shard IS the array. ROUTE_HOST: the shards come to the host ahead of the round, the whole array goes up to every
// rank. ROUTE_RCCL: one ncclAllGather of the shard buffers, padded to the largest shard, and unpad_kernel behind it.
#pragma once

namespace
{
// the padded all-gather layout [rank][largest shard][width] -> flat particle order (shard_layout.h holds the map)
__global__ void unpad_kernel(const float* __restrict__ padded, ShardLayout layout, size_t n, size_t width, float* __restrict__ flat)
{
  const size_t t = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= width * n)
    return;
  const size_t i = t / width, k = t % width;
  const ShardSlot at = shard_slot(layout, i);
  flat[t] = padded[(at.rank * shard_capacity(layout) + at.offset) * width + k];
}

// one rank's view of a sharded array
struct ShardedArray
{
  size_t width;              // floats per particle
  DevBuf* shard;             // the rank's shard, with room for the largest shard
  DevBuf* pad;               // where the padded all-gather lands
  DevBuf* flat;              // the whole array in particle order
  std::vector<float>* host;  // the group's host copy of the whole array (ROUTE_HOST)
  const char* name;          // in the error texts
  const char* nccl_call;
};

// ROUTE_HOST, ahead of the round: every shard of the resident particles' array `of(g, ctx)` describes, into its host vector
template <typename Of>
int gather_to_host(mcl3dl_hip_group* g, const Of& of)
{
  if (g->route() != ROUTE_HOST)
    return 0;
  of(g, g->ctx[0]).host->resize(of(g, g->ctx[0]).width * g->n_resident);
  return group_each_shard(g,
                          [&](mcl3dl_hip_ctx* ctx, int, size_t lo, size_t n) -> int
                          {
                            const ShardedArray a = of(g, ctx);
                            TRY(d2h(ctx, a.host->data() + a.width * lo, a.shard->p, sizeof(float) * a.width * n));
                            return sync_stream(ctx);
                          });
}

// in group_voted_call's `ahead`: room, the host-gathered array up, the all-gather's send count against the shard buffer
inline int gather_ahead(mcl3dl_hip_group* g, const Shard& s, size_t n_p, const ShardedArray& a)
{
  mcl3dl_hip_ctx* ctx = s.ctx;
  if (g->route() == ROUTE_DIRECT)
    return 0;
  const size_t row = sizeof(float) * a.width, cap = shard_capacity(n_p, g->n());
  TRY(ensure(ctx, *a.flat, row * n_p));
  if (g->route() == ROUTE_HOST)
    return h2d(ctx, a.flat->p, a.host->data(), row * n_p);
  TRY(ensure(ctx, *a.pad, row * cap * g->n()));
  if (a.shard->cap < row * cap)  // (every shard buffer holds the largest shard)
    return ctx->fail(-4, "internal: %s buffer smaller than the all-gather's send count", a.name);
  return 0;
}

// in `behind`: the all-gather over xGMI into the padded layout, then into particle order — or nothing. *whole: where the rank
// finds the array in particle order.
inline int gather_behind(mcl3dl_hip_group* g, const Shard& s, const VotedRank& voted, size_t n_p, const ShardedArray& a,
                         const float** whole)
{
  mcl3dl_hip_ctx* ctx = s.ctx;
  *whole = (g->route() == ROUTE_DIRECT ? a.shard : a.flat)->as<float>();
  if (g->route() != ROUTE_RCCL)
    return 0;
  const ShardLayout layout = shard_layout(n_p, g->n());
  const ncclResult_t nrc =
      g->rccl.AllGather(a.shard->p, a.pad->p, a.width * shard_capacity(layout), ncclFloat, g->comms[s.r], ctx->stream);
  TRY(voted.enqueued(nrc, a.nccl_call));
  hipLaunchKernelGGL(unpad_kernel, dim3(static_cast<unsigned>((a.width * n_p + 255) / 256)), dim3(256), 0, ctx->stream,
                     a.pad->as<float>(), layout, n_p, a.width, a.flat->as<float>());
  HIP_TRY(hipGetLastError());
  return 0;
}
}  // namespace
