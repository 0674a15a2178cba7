// tests/cpp/shard_layout_check.cpp — TEST INFRASTRUCTURE, plain C++ with nothing but mcl_3dl_amd/csrc/shard_layout.h: the
// shard bounds, the largest shard and the inverse map (particle -> rank, offset) the device group's host code and its unpad
// kernel share, written out for tests/test_shard_layout_cpu.py to hold against each other and against
// mcl_3dl_amd/distributed.py:shard_bounds.
//
//   shard_layout_check sweep <world_max> <n_max> <out>   uint32 words, for world = 1..world_max, n = 0..n_max:
//                                                        capacity, {lo, hi} per rank, {rank, offset} per particle
//   shard_layout_check edges <n> <world> <out>           uint64 words: capacity, then per rank lo, hi and {rank, offset} of
//                                                        its first and last particle (an empty shard: four zeros)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "shard_layout.h"

using namespace mcl3dl;

int main(int argc, char** argv)
{
  if (argc != 5)
    return 2;
  const bool sweep = !strcmp(argv[1], "sweep");
  if (!sweep && strcmp(argv[1], "edges"))
    return 2;
  const size_t a = strtoull(argv[2], nullptr, 10), b = strtoull(argv[3], nullptr, 10);
  std::vector<uint32_t> w32;
  std::vector<uint64_t> w64;
  if (sweep)
  {
    for (size_t world = 1; world <= a; ++world)
      for (size_t n = 0; n <= b; ++n)
      {
        w32.push_back(static_cast<uint32_t>(shard_capacity(n, world)));
        for (size_t r = 0; r < world; ++r)
        {
          size_t lo, hi;
          shard_bounds(n, static_cast<int>(world), static_cast<int>(r), &lo, &hi);
          w32.push_back(static_cast<uint32_t>(lo));
          w32.push_back(static_cast<uint32_t>(hi));
        }
        const ShardLayout layout = shard_layout(n, world);
        for (size_t i = 0; i < n; ++i)
        {
          const ShardSlot at = shard_slot(layout, i);
          w32.push_back(static_cast<uint32_t>(at.rank));
          w32.push_back(static_cast<uint32_t>(at.offset));
        }
      }
  }
  else
  {
    const size_t n = a, world = b;
    if (world < 1)
      return 2;
    const ShardLayout layout = shard_layout(n, world);
    w64.push_back(shard_capacity(layout));
    for (size_t r = 0; r < world; ++r)
    {
      size_t lo, hi;
      shard_bounds(n, static_cast<int>(world), static_cast<int>(r), &lo, &hi);
      w64.push_back(lo);
      w64.push_back(hi);
      const ShardSlot first = hi > lo ? shard_slot(layout, lo) : ShardSlot{ 0, 0 };
      const ShardSlot last = hi > lo ? shard_slot(layout, hi - 1) : ShardSlot{ 0, 0 };
      w64.insert(w64.end(), { first.rank, first.offset, last.rank, last.offset });
    }
  }
  FILE* f = fopen(argv[4], "wb");
  if (!f)
    return 3;
  const size_t want = sweep ? w32.size() : w64.size();
  const size_t wrote = sweep ? fwrite(w32.data(), sizeof(uint32_t), want, f) : fwrite(w64.data(), sizeof(uint64_t), want, f);
  return (fclose(f) == 0 && wrote == want) ? 0 : 3;
}
