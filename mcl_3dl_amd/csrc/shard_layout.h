// shard_layout.h — how n particles are split over the `world` ranks of a device group, stated once for the host code
// (host_group.h, the api_group_*.inl files) and for the kernel behind the padded all-gather (host_group_gather.h). Free of HIP and
// RCCL: tests/cpp/shard_layout_check.cpp includes it alone and holds the inverse map against the bounds for every world size a
// group accepts. Contiguous shards, the first n % world of them one longer: mcl_3dl_amd/distributed.py:shard_bounds' rule.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define MCL3DL_SHARD_HD __host__ __device__
#else
#define MCL3DL_SHARD_HD
#endif

namespace mcl3dl
{
struct ShardLayout
{
  size_t base, rem;  // n / world, n % world
};

MCL3DL_SHARD_HD inline ShardLayout shard_layout(size_t n, size_t world)
{
  return ShardLayout{ n / world, n % world };
}

// the largest shard: what EVERY rank's shard buffers hold room for, an empty rank's included (a padded all-gather sends that
// many from each rank)
MCL3DL_SHARD_HD inline size_t shard_capacity(const ShardLayout& l)
{
  return l.base + (l.rem ? 1 : 0);
}

MCL3DL_SHARD_HD inline size_t shard_capacity(size_t n, size_t world)
{
  return shard_capacity(shard_layout(n, world));
}

// contiguous shard [lo, hi) of rank r
MCL3DL_SHARD_HD inline void shard_bounds(size_t n, int world, int r, size_t* lo, size_t* hi)
{
  const ShardLayout l = shard_layout(n, static_cast<size_t>(world));
  const size_t rr = static_cast<size_t>(r);
  *lo = rr * l.base + (rr < l.rem ? rr : l.rem);
  *hi = *lo + l.base + (rr < l.rem ? 1 : 0);
}

// the inverse: the rank that holds particle i (i < n) and i's place in that rank's shard
struct ShardSlot
{
  size_t rank, offset;
};

MCL3DL_SHARD_HD inline ShardSlot shard_slot(const ShardLayout& l, size_t i)
{
  const size_t base = l.base, rem = l.rem;
  const size_t split = rem * (base + 1);  // the first `rem` shards hold base + 1 particles
  const size_t r = i < split ? i / (base + 1) : rem + (base ? (i - split) / base : 0);
  const size_t lo = r * base + (r < rem ? r : rem);
  return ShardSlot{ r, i - lo };
}
}  // namespace mcl3dl
