// term_slots.h — where the tiled likelihood kernel keeps a tile's 256 float terms of one particle in LDS (s_term[k][.]), for the
// kernel and for the CPU check of the mapping (tests/cpp/tiled_lean_check.cpp). Plain C++: no HIP type in here.
//
// The fixed-order fp64 sum gives a particle 256 / G lanes; lane t adds the SEG = G terms of segment s = t % (256 / G) in the
// order (j + t) % SEG, j = 0 .. SEG - 1 (a rotation that once kept its one-float LDS reads off each other's banks). For
// G = 4, 8, 16 SEG divides the lanes per particle, so the rotation is the segment's alone, (j + s) % SEG, and the WRITER can store
// the term of point i = s SEG + o where that reader meets it j-th: slot s SEG + ((o - s) mod SEG). The reader then takes its
// segment front to back, 16 bytes per LDS read and no address arithmetic between the reads — the same terms in the same
// order, so the same sum bit for bit.
// Banks (MI355X: a 16-byte LDS read is served in groups of 16 lanes, bank = (byte address / 4) mod 64): readers are SEG floats
// apart, so with SEG = 16 the lanes of a group would meet four to a bank, with SEG = 8 two. The 16-byte chunk a reader takes
// c-th is therefore chunk c ^ x(s) of its segment, x = (s >> 2) & 3 for SEG = 16 and (s >> 3) & 1 for SEG = 8: every group
// then covers the 64 banks once. A chunk stays inside its segment, so a wavefront's store of one term per lane (a 4-byte LDS
// write, groups of 32 lanes, bank = (byte address / 4) mod 32) still covers 32 consecutive floats per group.
// G = 32 (SEG = 32 does not divide its 8 lanes per particle) and the float chain (chain_add_row adds in array order) keep the
// array order: term_slot<G, false> is the identity for them.
#pragma once

#if defined(__HIPCC__)
#define MCL3DL_SLOT_HD __host__ __device__
#else
#define MCL3DL_SLOT_HD
#endif

namespace mcl3dl
{
// are the terms of this instantiation stored in the reader's order?
template <int G, bool CHAIN>
struct TermSlots
{
  static constexpr bool permuted = !CHAIN && (G == 4 || G == 8 || G == 16);
  static constexpr int SEG = G;  // terms per reader lane
};

// the reader's chunk swizzle of segment s (in 16-byte chunks)
template <int G>
MCL3DL_SLOT_HD constexpr int term_chunk_xor(int s)
{
  return G == 16 ? ((s >> 2) & 3) : G == 8 ? ((s >> 3) & 1) : 0;
}

// slot of the term of point i (0 .. 255) in its particle's row
template <int G, bool CHAIN>
MCL3DL_SLOT_HD constexpr int term_slot(int i)
{
  if (!TermSlots<G, CHAIN>::permuted)
    return i;
  const int s = i / G, o = i % G;
  return (s * G + ((o - s) & (G - 1))) ^ (term_chunk_xor<G>(s) << 2);
}

// slot the reader of segment s takes j-th (j = 0 .. SEG - 1): chunk by chunk, the chunks in the swizzled order
template <int G>
MCL3DL_SLOT_HD constexpr int term_read_slot(int s, int j)
{
  return (s * G + j) ^ (term_chunk_xor<G>(s) << 2);
}
}  // namespace mcl3dl
