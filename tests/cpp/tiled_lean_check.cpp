// tiled_lean_check.cpp — CPU check of the tiled likelihood kernel's term slots (mcl_3dl_amd/csrc/term_slots.h), a stand-alone
// program: for G = 4, 8, 16
//   * the slot mapping is a bijection on [0, 256);
//   * for every reader lane t and j, the slot read j-th holds the term of point seg SEG + (j + t) % SEG — the sequence the
//     fp64 sum has always added in;
//   * the kernel's own index expression (first ^ c, in 16-byte chunks) names those slots;
//   * a wavefront's 4-byte stores of one pose touch 32 distinct banks per half wavefront (bank = float index mod 32);
//   * every 16-byte read is conflict-free within each of the four lane groups a wave64 16-byte LDS read is served in
//     ({0-3,12-15,20-27}, {4-11,16-19,28-31}, the same + 32; bank = float index mod 64, four consecutive banks per lane);
// and G = 32 and the float chain keep the array order.
#include <cstdio>
#include <set>
#include <vector>

#include "term_slots.h"

using namespace mcl3dl;

static int failures = 0;
#define CHECK(cond, ...)                                                                                                          \
  do                                                                                                                              \
  {                                                                                                                               \
    if (!(cond))                                                                                                                  \
    {                                                                                                                             \
      if (++failures <= 20)                                                                                                       \
      {                                                                                                                           \
        std::printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #cond);                                                              \
        std::printf(__VA_ARGS__);                                                                                                 \
        std::printf("\n");                                                                                                        \
      }                                                                                                                           \
    }                                                                                                                             \
  } while (0)

// the lane groups of a 16-byte LDS read
static int read_group(int lane)
{
  const int half = lane >> 5, l = lane & 31;
  const bool first = l < 4 || (l >= 12 && l < 16) || (l >= 20 && l < 28);
  return half * 2 + (first ? 0 : 1);
}

template <int G>
static void check_permuted()
{
  constexpr int LPP = 256 / G, SEG = G, LD = 256;
  static_assert(TermSlots<G, false>::permuted && !TermSlots<G, true>::permuted, "which instantiations permute");
  // bijection
  std::set<int> seen;
  for (int i = 0; i < 256; ++i)
  {
    const int sl = term_slot<G, false>(i);
    CHECK(sl >= 0 && sl < 256, "G %d point %d slot %d", G, i, sl);
    seen.insert(sl);
    CHECK((term_slot<G, true>(i)) == i, "G %d: the chain keeps the array order (point %d)", G, i);
  }
  CHECK(seen.size() == 256u, "G %d: %zu distinct slots", G, seen.size());
  // the reader's sequence, and the kernel's index expression
  for (int t = 0; t < 256; ++t)
  {
    const int seg = t % LPP;
    for (int j = 0; j < SEG; ++j)
    {
      const int point = seg * SEG + (j + t) % SEG;
      CHECK((term_slot<G, false>(point)) == term_read_slot<G>(seg, j), "G %d lane %d j %d: point %d at slot %d, read slot %d", G, t, j,
            point, term_slot<G, false>(point), term_read_slot<G>(seg, j));
    }
    const int first = (seg * (SEG / 4)) ^ term_chunk_xor<G>(seg);
    for (int c = 0; c < SEG / 4; ++c)
      CHECK((first ^ c) * 4 == term_read_slot<G>(seg, 4 * c), "G %d lane %d chunk %d: kernel index %d, slot %d", G, t, c, (first ^ c) * 4,
            term_read_slot<G>(seg, 4 * c));
  }
  // stores: lane l of wavefront w holds point 64 w + l and writes row k at its slot
  for (int w = 0; w < 4; ++w)
    for (int half = 0; half < 2; ++half)
    {
      std::set<int> banks;
      for (int l = 0; l < 32; ++l)
        banks.insert(term_slot<G, false>(64 * w + 32 * half + l) % 32);
      CHECK(banks.size() == 32u, "G %d wavefront %d half %d: %zu banks written", G, w, half, banks.size());
    }
  // reads: lane t of the work-group reads row pk = t / LPP, segment t % LPP, chunk by chunk
  for (int w = 0; w < 4; ++w)
    for (int c = 0; c < SEG / 4; ++c)
    {
      std::vector<std::set<int>> banks(4);
      std::vector<int> lanes(4, 0);
      for (int l = 0; l < 64; ++l)
      {
        const int t = 64 * w + l, pk = t / LPP, seg = t % LPP;
        const int at = pk * LD + term_read_slot<G>(seg, 4 * c);  // float index in s_term
        CHECK(at % 4 == 0, "G %d lane %d chunk %d: a 16-byte read at float %d", G, t, c, at);
        for (int d = 0; d < 4; ++d)
          banks[read_group(l)].insert((at + d) % 64);
        ++lanes[read_group(l)];
      }
      for (int g = 0; g < 4; ++g)
        CHECK(lanes[g] == 16 && banks[g].size() == 64u, "G %d wavefront %d chunk %d group %d: %d lanes on %zu banks", G, w, c, g, lanes[g],
              banks[g].size());
    }
  std::printf("term slots G = %d: ok\n", G);
}

int main()
{
  check_permuted<4>();
  check_permuted<8>();
  check_permuted<16>();
  static_assert(!TermSlots<32, false>::permuted && !TermSlots<32, true>::permuted, "G = 32 keeps the array order");
  for (int i = 0; i < 256; ++i)
    CHECK((term_slot<32, false>(i)) == i, "G 32 point %d", i);
  if (failures)
  {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
