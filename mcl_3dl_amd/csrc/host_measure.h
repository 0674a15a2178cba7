// host_measure.h — part of the single translation unit mcl3dl_hip.hip: parameter structs for the kernels, the rules that
// choose among them (each written once), plan_measure — every decision, size check and buffer of a scan update, before anything
// is enqueued — and launch_measure with one small launcher per route, the one place that enqueues the likelihood and beam kernels.
#pragma once
#include <type_traits>

namespace
{
int ensure_structures(mcl3dl_hip_ctx* ctx, bool need_lik, bool need_dda, bool need_cells = false)
{
  if (!ctx->has_map)
    return ctx->fail(-5, "no map: call mcl3dl_hip_set_map first");
  bool built = false;
  // a cell grid laid out for the kd-tree caster's radius (lik_cell_edge) does not serve the likelihood model's 27-cell
  // search: that model running on its default parameters counts as having set them
  if (need_lik && ctx->opt.lik_index == 0 && !need_cells && !ctx->lik_params_set && (ctx->lik_cell_from_beam || lik_cell_is_beams(ctx)))
  {
    ctx->lik_params_set = true;
    if (ctx->lik_cell_from_beam)
      ctx->lik_dirty = ctx->lik_base_dirty = true;
  }
  if (need_lik && (ctx->opt.lik_index == 0 || need_cells) && ctx->lik_dirty)
  {
    TRY(build_lik_grid(ctx));
    built = true;
  }
  // the 27-cell scan rests on the cell edge's 1 % margin over the radius, which the float rounding of the cell coordinates
  // uses up at LIK_SCAN_MAX_CELLS cells per axis (index_geometry.h); radius searches scan a cell more each way and go on
  if (need_lik && ctx->opt.lik_index == 0 && !need_cells)
  {
    const int dim[3] = { ctx->lg.nx, ctx->lg.ny, ctx->lg.nz };
    if (!lik_scan_provable(dim))
      return ctx->fail(-4, "the map's cell grid has %d x %d x %d cells: the 27-cell scan (lik_index 0) is exact up to %d cells per "
                           "axis; use lik_index 2", dim[0], dim[1], dim[2], LIK_SCAN_MAX_CELLS);
  }
  if (need_lik && ctx->opt.lik_index >= 1 && !need_cells && ctx->cand_dirty)
  {
    TRY(build_cand_grid(ctx));
    built = true;
  }
  if (need_dda && ctx->dda_dirty)
  {
    TRY(build_dda_grid(ctx));
    built = true;
  }
  if (built)
    scratch_trim(ctx, 64u << 20);  // the temporaries of a whole-map build do not stay parked (map updates keep their small ones)
  return 0;
}

// RaycastUsingKDTree's constants for the cell grid in place (ensure_caster_structures has run).
KdRayParams kd_ray_params(const mcl3dl_hip_ctx* ctx)
{
  KdRayParams k;
  float r1, r2;
  kd_ray_radii(ctx, &k.grid_min, &r1, &r2);
  k.hit_tolerance = ctx->hit_range;
  k.two_grid_min = k.grid_min * 2.0;
  // pcl::KdTreeFLANN::radiusSearch: (float)(radius * radius) with radius widened to double
  k.r1_sq = static_cast<float>(static_cast<double>(r1) * static_cast<double>(r1));
  k.r2_sq = static_cast<float>(static_cast<double>(r2) * static_cast<double>(r2));
  // cells each way that hold every point within the radius: ceil(r / cell), with half a percent of a cell for the float
  // rounding of the binning expression (the grid's own edge is 1 % over the radius it is laid out for)
  const double cell = 1.0 / static_cast<double>(ctx->lg.inv_cell);
  const auto reach = [&](float r) { return static_cast<int>(std::min(std::ceil(static_cast<double>(r) / cell + 0.005), 1.0e6)); };
  k.reach1 = reach(r1);
  k.reach2 = reach(r2);
  k.wx = ctx->weight[0];
  k.wy = ctx->weight[1];
  k.wz = ctx->weight[2];
  k.has_weight = ctx->has_weight ? 1 : 0;
  k.map = ctx->map_dev.as<float4>();
  k.occ = ctx->kd_occ.as<uint32_t>();
  return k;
}

// What the beam model's caster needs before it casts (need_beam: there are rays): the DDA grid for RaycastUsingDDA; for
// RaycastUsingKDTree the cell-sorted map — whatever the likelihood model's index is, and also when that model never runs —
// and the map itself on the device (labels, unscaled points). A context on the kd-tree caster never builds the DDA grid here.
int ensure_caster_structures(mcl3dl_hip_ctx* ctx, bool need_lik, bool need_beam, bool need_cells = false)
{
  if (ctx->beam_raycast != 1)
    return ensure_structures(ctx, need_lik, need_beam, need_cells);
  TRY(ensure_structures(ctx, need_lik, false, need_cells));
  if (need_beam)
  {
    if (ctx->lik_dirty)
    {
      TRY(build_lik_grid(ctx));
      scratch_trim(ctx, 64u << 20);
    }
    TRY(ensure_map_dev(ctx));
    // the dilated occupancy bitmap of this grid, for this reach of the first search (a map update's merge, a new cell edge,
    // other map_grid sizes: built again — one pass over the run delimiters)
    const KdRayParams k = kd_ray_params(ctx);
    if (ctx->kd_occ_reach != k.reach1)
    {
      const unsigned long long n_cells = static_cast<unsigned long long>(ctx->lg.nx) * ctx->lg.ny * ctx->lg.nz;
      const unsigned long long blocks = (n_cells + 255) / 256;
      if (blocks > 0x7fffffffull)
        return ctx->fail(-4, "the cell grid has too many cells for the kd-tree caster's occupancy bitmap");
      TRY(ensure(ctx, ctx->kd_occ, sizeof(unsigned long long) * ((n_cells + 63) / 64)));
      hipLaunchKernelGGL(kd_occupancy_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, ctx->stream, ctx->lg, k.reach1,
                         n_cells, ctx->kd_occ.as<unsigned long long>());
      HIP_TRY(hipGetLastError());
      ctx->kd_occ_reach = k.reach1;
    }
  }
  return 0;
}

// Page-locked, device-mapped arrays the last kernel of an update writes its results to (each may be null).
using HostOut = PfEmit;

LikParams lik_params(const mcl3dl_hip_ctx* ctx)
{
  LikParams p;
  p.wx = ctx->weight[0];
  p.wy = ctx->weight[1];
  p.wz = ctx->weight[2];
  p.has_weight = ctx->has_weight ? 1 : 0;
  p.unit_form = lik_unit_form(p.wx, p.wy, p.wz);
  p.match_dist_min = ctx->match_dist_min;
  // pcl::KdTreeFLANN::radiusSearch: (float)(radius * radius) with radius widened to double
  p.r2 = static_cast<float>(static_cast<double>(ctx->match_dist_min) * static_cast<double>(ctx->match_dist_min));
  p.match_dist_flat = ctx->match_dist_flat;
  p.match_weight = ctx->match_weight;
  return p;
}

BeamParams beam_params(const mcl3dl_hip_ctx* ctx)
{
  BeamParams p;
  p.sin_total_ref = ctx->sin_total_ref;
  p.hit_range_sq = ctx->hit_range_sq;
  p.filter_label_max = ctx->filter_label_max;
  p.short_only = ctx->short_only;
  p.beam_likelihood_min = ctx->beam_likelihood_min;
  return p;
}

// LidarMeasurementModelBeam::refreshParameters, src/lidar_measurement_model_beam.cpp:65-67 (host libm, like the reference)
void beam_refresh(mcl3dl_hip_ctx* ctx)
{
  ctx->hit_range_sq = static_cast<float>(std::pow(static_cast<double>(ctx->hit_range), 2));
  ctx->beam_likelihood = static_cast<float>(
      std::pow(static_cast<double>(ctx->beam_likelihood_min), 1.0 / static_cast<float>(ctx->beam_num_points)));
  ctx->sin_total_ref = sinf(ctx->ang_total_ref);
  ctx->pow_table_dirty = true;
}

// table[k] = score_beam after k penalised rays: `score_beam *= beam_likelihood_` repeated k times (beam.cpp:148), float. Built
// for at least 1024 counts so that alternating scan sizes (the adapter launches the two models separately) do not rebuild it
// every update.
// n_b_coming: the beam scan size of an update whose scan is not in the context yet (0: the current one)
int ensure_pow_table(mcl3dl_hip_ctx* ctx, size_t n_b_coming = 0)
{
  const size_t n_b = std::max(ctx->n_b, n_b_coming);
  if (!(ctx->pow_table_dirty || n_b > ctx->pow_table_len))
    return 0;
  const size_t len = std::max<size_t>(n_b, 1024);
  std::vector<float> table(len + 1);
  table[0] = 1.0f;
  for (size_t k = 1; k <= len; ++k)
    table[k] = table[k - 1] * ctx->beam_likelihood;
  TRY(ensure(ctx, ctx->pow_table, sizeof(float) * table.size()));
  TRY(h2d(ctx, ctx->pow_table.p, table.data(), sizeof(float) * table.size()));
  TRY(sync_stream(ctx));
  ctx->pow_table_dirty = false;
  ctx->pow_table_len = len;
  return 0;
}

// ---- compile-time dispatch: a runtime value picks the template instance (each list names every instance there is) ------
// f(std::integral_constant<int, V>) for the V that equals v; the LAST value listed also takes whatever matches none
template <int V, int... Rest, class F>
void dispatch_int(int v, F&& f)
{
  if constexpr (sizeof...(Rest) > 0)
    if (v != V)
      return dispatch_int<Rest...>(v, f);
  f(std::integral_constant<int, V>{});
}

// Scans up to this many points fit the caller-order term row of the per-particle kernels (48 KB of the 64 KB of LDS a
// work-group gets without asking for more).
constexpr int LIK_ROW_MAX = 12288;

// Which likelihood kernel family a launch of np particles x ns points takes, and how its terms are added (no allocation:
// plan_lik and the one-launch update both ask).
//   exact   the sum must be the reference's float, in the caller's order: strict_order 1 always; the default (2) for every
//           scan of at most strict_exact_max points (4096: the reference's operating range and far beyond — the fuzz's gate is
//           assert_array_equal there) and from strict_auto_min points up, where the reference's own float rounding is no longer
//           safely inside north_star's 1e-5 (host_context.h); in between, and with strict_order 0, the fixed-order fp64 tree
//   rows    ... by the per-particle kernels themselves: every term parked in LDS at its ORIGINAL scan index, one wavefront
//           runs the recurrence (lik_particle / likelihood_small_kernel) — no term array, no second launch
//   replay  ... by the tiled kernel + the N_s x N_p term array + lik_strict_sum_rows_kernel
// Measured (profiles/r06d_rows_vs_replay.txt): below ~2000 particles the rows are the cheaper exact form at every scan size
// that fits them (64 x 4096: 21 against 38 us; 1024 x 4096: 48 against 58), above it the replay (4096 x 4096: 116 against 126).
struct LikMode
{
  bool tiled = false, rows = false, replay = false;
};

LikMode lik_mode(const mcl3dl_hip_ctx* ctx, int np, int ns)
{
  LikMode m;
  // tiled from lik_tiled_min points up (default 1024), and already from three quarters of that when there are enough particles
  // to fill the GPU with (tile, group) pairs (4096 x 1000: 30.6 us tiled against 34.9 us; 64 x 1000 and 4096 x 512: no gain)
  const bool by_size = ctx->opt.lik_tiled && np >= 4 &&
                       (ns >= ctx->opt.lik_tiled_min || (np >= 256 && 4 * static_cast<long long>(ns) >= 3ll * ctx->opt.lik_tiled_min));
  if (ctx->opt.strict_order == 3)
  {
    m.tiled = true;  // the in-kernel chain, in the engine's scan order
    return m;
  }
  const bool exact = ctx->opt.strict_order == 1 ||
                     (ctx->opt.strict_order == 2 && (ns <= ctx->opt.strict_exact_max || ns >= ctx->opt.strict_auto_min));
  // (a scan ordered in chunks of the caller's order — option strict_chunk — carries chunk-relative indices: the replay's business)
  const bool rows_fit = ns <= LIK_ROW_MAX && ctx->scan_chunk == 0;
  if (!exact)
  {
    m.tiled = by_size;
    // where a per-particle kernel runs anyway the rows cost a few per cent: exact there too (unless told not to: strict_order 0)
    m.rows = !by_size && ctx->opt.strict_order == 2 && rows_fit;
    return m;
  }
  if (rows_fit && (!by_size || np < STRICT_ROWS_MAX_PARTICLES))
    m.rows = true;
  else
    m.tiled = m.replay = true;
  return m;
}

// the small-scan kernel (likelihood_small_kernel: W lanes per particle) takes what the tiled kernel leaves of short scans
bool lik_small_applies(const mcl3dl_hip_ctx* ctx, const LikMode& m, int np, int ns)
{
  return !m.tiled && ns <= 32 && np >= 256 && ctx->opt.lik_small;
}

// the likelihood kernels' cooperative form: its sqrt needs match_dist_min > 1.2e-7 m (likelihood_kernels.h:sqrt_in_radius)
bool lik_coop_active(const mcl3dl_hip_ctx* ctx)
{
  return ctx->opt.lik_coop && ctx->opt.lik_index == 2 && ctx->match_dist_min > 1e-5f;
}

// Work-group size of the per-particle likelihood kernel — and of whatever carries it (lik_particle_beam_kernel, the one-launch
// update): the same everywhere, so that the lanes add in the same order.
int lik_particle_block(const mcl3dl_hip_ctx* ctx, int np, int ns)
{
  if (ns <= 128)
    return 64;
  // few particles: 16 wavefronts share a scan — a quarter of the dependent load chains per lane
  if (ctx->opt.lik_index == 2 && np <= LIK_WIDE_MAX_PARTICLES && ns > 512)
    return 1024;
  return 256;
}

// (BLOCK, MODE) of the per-particle kernels: the 1024-thread form exists for MODE 2 only
template <class F>
void dispatch_particle(int block, int mode, F&& f)
{
  if (mode == 2)
    dispatch_int<64, 1024, 256>(block, [&](auto b) { f(b, std::integral_constant<int, 2>{}); });
  else
    dispatch_int<64, 256>(block, [&](auto b) { f(b, std::integral_constant<int, 0>{}); });
}

// Work-groups of the tiled kernel over n_tiles tiles of 256 points — per XCD: the interleaved tiles of the largest multiple of
// eight, then an eighth of the remaining (tile, group) pairs
long long tiled_blocks(int n_tiles, int n_groups)
{
  const long long full_tiles = n_tiles & ~7, rem_items = static_cast<long long>(n_tiles - full_tiles) * n_groups;
  return 8 * ((full_tiles / 8) * n_groups + (rem_items + 7) / 8);
}

// A launch of both models: rounds of beam8 x 8 beam work-groups + other8 x 8 of the likelihood kernel's, beam8 : other8 ~ the
// two grids' ratio (each at most 8); grid = work-groups of the whole launch
struct Interleave
{
  uint32_t beam8 = 1, other8 = 1;
  long long grid = 0;
};

Interleave interleave(long long n_beam, long long n_other)
{
  Interleave il;
  if (n_beam >= n_other)
    il.beam8 = static_cast<uint32_t>(std::min<long long>(8, (n_beam + n_other / 2) / n_other));
  else
    il.other8 = static_cast<uint32_t>(std::min<long long>(8, (n_other + n_beam / 2) / n_beam));
  const long long rounds = std::max((n_beam + 8 * il.beam8 - 1) / (8 * il.beam8), (n_other + 8 * il.other8 - 1) / (8 * il.other8));
  il.grid = rounds * 8 * (il.beam8 + il.other8);
  return il;
}

// the tiled kernel with its overflow rounds deferred (likelihood_kernels.h): needs packed 64-byte records; mode 2 = only
// on maps where enough voxels overflow for a wavefront to meet one in nearly every round
bool lik_defer_active(const mcl3dl_hip_ctx* ctx)
{
  if (ctx->opt.lik_defer == 0 || ctx->opt.lik_index != 2 || !ctx->rg.packed || ctx->rg.rec_parts != 4)
    return false;
  if (ctx->opt.lik_defer == 1)
    return true;
  const double with_cand = ctx->cand_stats[4], over4 = ctx->cand_stats[5];
  return with_cand > 0 && over4 / with_cand > LIK_DEFER_MIN_FRAC;
}

// the tiled kernel's pose loop specialised for the common map (RecGrid::common_map): taken by the deferred form when the map
// is one, the parameters let `matched` follow from the radius test, and nobody switched it off
bool lik_tiled_fast_active(const mcl3dl_hip_ctx* ctx, const LikParams& p)
{
  return ctx->opt.lik_tiled_fast != 0 && ctx->rg.common_map && lik_defer_active(ctx) && lik_coop_active(ctx) &&
         lik_match_from_radius(p.match_dist_min, p.r2, p.match_dist_flat);
}

// the record grid as a launch of the tiled kernel gets it: common_map says which pose loop the launch runs
RecGrid tiled_rec_grid(const mcl3dl_hip_ctx* ctx, const LikParams& p)
{
  RecGrid rg = ctx->rg;
  rg.common_map = lik_tiled_fast_active(ctx, p) ? 1 : 0;
  return rg;
}

// hand-off words + error word of the in-kernel chain for n_p particles and n_tiles tiles; *tag0 = tag of tile 0
int ensure_chain(mcl3dl_hip_ctx* ctx, size_t n_p, int n_tiles, uint32_t* tag0)
{
  if (!ctx->chain_err)
  {
    // (the word is kept only once the platform has shown that the device can write it in place: a context on a platform
    // without such memory fails HERE on every call instead of launching kernels that write through a pointer the device
    // cannot reach — ADVICE round 5)
    volatile unsigned* w = ctx->zero_copy_supported ? static_cast<volatile unsigned*>(pinned_alloc(ctx, 64)) : nullptr;
    if (!w || !ctx->zero_copy_supported)
      return ctx->fail(-2, "strict_order = 3 needs page-locked memory the device can write in place");
    *w = 0u;
    ctx->chain_err = w;
  }
  const size_t need = sizeof(unsigned long long) * 2 * n_p;
  const bool fresh = need > ctx->chain_carry.cap;
  TRY(ensure(ctx, ctx->chain_carry, need));
  // tags only grow; a fresh buffer (or a wrap of the 32-bit tag) starts from cleared words and tag 1
  if (fresh || ctx->chain_tag > 0xffffffffu - static_cast<uint32_t>(n_tiles) - 2u)
  {
    HIP_TRY(hipMemsetAsync(ctx->chain_carry.p, 0, ctx->chain_carry.cap, ctx->stream));
    ctx->chain_tag = 1u;
  }
  *tag0 = ctx->chain_tag;
  ctx->chain_tag += static_cast<uint32_t>(n_tiles) + 1u;
  return 0;
}

// strict_order = 3 launches of ONE device are serialised across contexts: the hand-off makes progress only while a
// consumer's producer is resident or done, which dispatch in block-index order guarantees inside one launch — but two chain kernels
// running side by side (two contexts, or two ranks of a device group on one GPU) could fill each other's XCDs with polling
// consumers (bounded: ~1 s, then error -2). A process-wide event per device: a chain launch waits for the previous one's.
struct ChainSerial
{
  std::mutex m;
  hipEvent_t ev = nullptr;
};
inline ChainSerial& chain_serial(int device)
{
  static ChainSerial per_device[64];
  return per_device[(device >= 0 && device < 64) ? device : 0];
}

// rows of G floats per particle group: what the float-order replay of ns points x n_p particles stores
size_t strict_terms_bytes(size_t n_p, int ns, int group_size)
{
  const size_t G = static_cast<size_t>(group_size);
  return ((n_p + G - 1) / G) * (sizeof(float) * static_cast<size_t>(ns) * G + sizeof(float4) * STRICT_SKEW4);
}

// device memory of the float-order replay: the whole scan's terms, or two chunks' when the scan was ordered in chunks
size_t strict_plan_bytes(const mcl3dl_hip_ctx* ctx, size_t n_p, int ns, int group_size)
{
  if (ctx->scan_chunk && static_cast<size_t>(ns) > ctx->scan_chunk)
    return 2 * strict_terms_bytes(n_p, static_cast<int>(ctx->scan_chunk), group_size);
  return strict_terms_bytes(n_p, ns, group_size);
}

int ensure_replay_stream(mcl3dl_hip_ctx* ctx)
{
  if (!ctx->replay_stream)
    HIP_TRY(hipStreamCreateWithFlags(&ctx->replay_stream, hipStreamNonBlocking));
  for (int k = 0; k < 2; ++k)
  {
    if (!ctx->ev_tiled[k])
      HIP_TRY(hipEventCreateWithFlags(&ctx->ev_tiled[k], hipEventDisableTiming));
    if (!ctx->ev_replay[k])
      HIP_TRY(hipEventCreateWithFlags(&ctx->ev_replay[k], hipEventDisableTiming));
  }
  return 0;
}

int plan_group_size(const mcl3dl_hip_ctx* ctx, int np, int ns)
{
  // particles per work-group of the tiled kernel: the largest of 16 / 8 / 4 that still gives the 256 CUs x 8
  // work-group slots something to do (few particles x a long scan would otherwise leave most of the GPU idle)
  int group_size = ctx->opt.lik_group;
  if (group_size == 0)
  {
    const long long n_tiles_ll = (ns + 255) / 256;
    group_size = 4;
    for (int gg = 16; gg >= 4; gg >>= 1)
      if (n_tiles_ll * ((np + gg - 1) / gg) >= 2048)
      {
        group_size = gg;
        break;
      }
  }
  return group_size;
}

// ---- the plan of one launch_measure call ------------------------------------------------------------------------------
enum class LikRoute
{
  None,        // no likelihood output asked for
  Ones,        // no scan points: (1, 0) for every particle by fill_kernel
  Small,       // likelihood_small_kernel<W, MODE>
  Tiled,       // likelihood_tiled_kernel<G, MODE, MINW, COOP, DEFER> + lik_finalize_kernel / the caller's tail kernel / the replay
  Chain,       // likelihood_tiled_kernel<G, MODE, 8, COOP, DEFER, CHAIN>: the float sum in the scan array's order inside the kernel
  ChainMulti,  // likelihood_chain_multi_kernel: four tiles per work-group (n_super super-tiles)
  Particle     // likelihood_kernel<BLOCK, MODE>
};

enum class BeamRoute
{
  None,            // no beam output asked for
  OnesByFill,      // no beam points: ones by fill_kernel
  OnesByFinalize,  // ... by whatever finishes the tiled likelihood kernel's sums
  Main,            // a launch of its own on the context's stream
  Aux,             // ... on the second stream, forked and joined (mcl3dl_hip_ctx::aux_stream)
  MergedTiled,     // its work-groups ride in the tiled likelihood kernel's launch (lik_beam_kernel)
  MergedChain,     // ... in the tiled kernel's in-kernel-chain form (strict_order 3)
  MergedParticle   // ... in the per-particle likelihood kernel's (lik_particle_beam_kernel)
};

// Every decision of one call — which kernels run, on which streams, with which template arguments — with every size check and
// every buffer the launches need done by plan_measure: before launch_measure forks the beam kernels onto the second stream, so
// that no error path can return with un-joined work in flight.
struct MeasurePlan
{
  LikRoute lik = LikRoute::None;
  // are the likelihoods of this launch the reference's floats bit for bit (caller-order rows, the float-order replay, the
  // in-kernel chain, or no terms at all)? pf::measure then adds the weights as the reference does, too (pf_float_order)
  bool lik_exact = false;
  int mode = 0;                      // MODE: 2 = candidate records (lik_index 2), 0 = cell search
  bool coop = false, defer = false;  // COOP, DEFER (the latter for the tiled routes only)
  int group_size = 16;               // G (MINW follows from it: 4 for 32, else 8)
  int W = 1, block = 256;            // lanes per particle of the small-scan kernel; the per-particle kernel's work-group size
  int n_tiles = 0, n_groups = 0, n_super = 0;
  long long blocks = 0;
  float* strict_terms = nullptr;
  size_t chunk = 0;    // > 0: the scan is ordered in chunks of the caller's order and replayed chunk by chunk (two term buffers)
  uint32_t chain_tag0 = 0;
  bool rows = false;   // per-particle / small-scan kernel with the terms parked in LDS at their ORIGINAL scan indices and added up
                       // as the reference adds them (float, sequentially, caller's order): bit-identical likelihoods
  BeamRoute beam = BeamRoute::None;
  bool kd = false;        // RaycastUsingKDTree (beam_kd_kernel) instead of the DDA walk
  bool prepared = false;  // beam_origin_kernel first: what depends only on (particle, origin), once per pair
  long long n_rays = 0, beam_blocks = 0;
  bool replay_is_long = false;

  bool chain() const
  {
    return lik == LikRoute::Chain || lik == LikRoute::ChainMulti;
  }
  bool tiled() const
  {
    return lik == LikRoute::Tiled || chain();
  }
};

// The AUTOMATIC replay (scans of at least strict_auto_min points) costs ns x n_p floats of device memory — 0.5 GB at
// 32 768 x 4096, 26 GB at 65 536 x 100 000. It is a refinement (the fp64 sums are within ~1e-5 of the reference's
// float at such sizes), so it must never make an update fail: when the buffer would take more than half of the free
// device memory, or its allocation fails, this launch sums in fp64 like smaller scans do. (strict_order = 1 — asked for
// explicitly — still fails loudly.)
bool auto_replay_affordable(mcl3dl_hip_ctx* ctx, size_t need)
{
  const bool over_cap = ctx->opt.strict_auto_max_bytes > 0.0 && static_cast<double>(need) > ctx->opt.strict_auto_max_bytes;
  if (!over_cap && need <= ctx->strict_terms.cap)
    return true;
  if (!over_cap)
  {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess)
    {
      (void)hipGetLastError();
      free_b = 0;
    }
    if (need + need / 4 <= (free_b + ctx->strict_terms.cap) / 2 && ensure(ctx, ctx->strict_terms, need) == 0)
      return true;
    (void)hipGetLastError();
    ctx->err.clear();
  }
  ++ctx->strict_auto_skipped;
  return false;
}

// strict_order = 3: the reference's float recurrence over the scan in the ENGINE's order (mcl3dl_hip_scan_order), inside the
// tiled kernel — no term array, no replay: the chain forms' grids and hand-off words (ensure_chain: with a page-locked error word)
int plan_chain(mcl3dl_hip_ctx* ctx, size_t n_p, MeasurePlan* pl)
{
  const int np = static_cast<int>(n_p);
  // few particles on a long scan (default kernel family only): four tiles per work-group, a quarter of the hand-offs
  // (likelihood_chain_multi.h). chain_ppl: 0 = by size, 1 = never, 4 = whenever the family allows.
  const bool family = pl->coop && pl->defer && ctx->opt.lik_group == 0;
  int n_handoffs = pl->n_tiles;
  if (family && (ctx->opt.chain_ppl == 4 || (ctx->opt.chain_ppl == 0 && pl->n_tiles >= 16 && np <= CHAIN_MULTI_MAX)))
  {
    pl->lik = LikRoute::ChainMulti;
    pl->group_size = 4;
    pl->n_groups = (np + 3) / 4;
    n_handoffs = pl->n_super = (pl->n_tiles + 3) / 4;
    pl->blocks = 8ll * ((pl->n_super + 7) / 8) * pl->n_groups;
  }
  else
  {
    // rows of eight tiles, no shared-out remainder (likelihood_tiled_kernel<..., CHAIN>)
    pl->lik = LikRoute::Chain;
    pl->blocks = 8ll * ((pl->n_tiles + 7) / 8) * pl->n_groups;
  }
  if (pl->blocks > 0x7fffffffLL)
    return ctx->fail(-3, "too many work-groups for the tiled likelihood kernel");
  return ensure_chain(ctx, n_p, n_handoffs, &pl->chain_tag0);
}

// the likelihood side of the plan for np particles x ns > 0 points
int plan_lik(mcl3dl_hip_ctx* ctx, size_t n_p, int ns, MeasurePlan* pl)
{
  const int np = static_cast<int>(n_p);
  const LikMode mode = lik_mode(ctx, np, ns);
  pl->rows = mode.rows;
  pl->mode = ctx->opt.lik_index == 2 ? 2 : 0;
  pl->coop = lik_coop_active(ctx);
  pl->group_size = plan_group_size(ctx, np, ns);
  const bool chain = ctx->opt.strict_order == 3;
  if (chain && pl->group_size > 16)
    pl->group_size = 16;
  const bool strict = mode.replay && (ctx->opt.strict_order != 2 || auto_replay_affordable(ctx, strict_plan_bytes(ctx, n_p, ns, pl->group_size)));
  if (lik_small_applies(ctx, mode, np, ns))
  {
    pl->lik = LikRoute::Small;
    while (pl->W < ns)
      pl->W <<= 1;
    pl->blocks = (static_cast<long long>(np) * pl->W + 255) / 256;
    if (pl->blocks > 0x7fffffffLL)
      return ctx->fail(-3, "too many work-groups for the small-scan likelihood kernel");
    return 0;
  }
  if (!mode.tiled)
  {
    pl->lik = LikRoute::Particle;
    pl->block = lik_particle_block(ctx, np, ns);
    return 0;
  }
  pl->lik = LikRoute::Tiled;
  pl->defer = pl->coop && lik_defer_active(ctx);
  pl->n_tiles = (ns + 255) / 256;
  pl->n_groups = (np + pl->group_size - 1) / pl->group_size;
  if (chain)
    return plan_chain(ctx, n_p, pl);
  pl->blocks = tiled_blocks(pl->n_tiles, pl->n_groups);
  if (pl->blocks > 0x7fffffffLL)
    return ctx->fail(-3, "too many work-groups for the tiled likelihood kernel");
  TRY(ensure(ctx, ctx->lik_partial_sum, sizeof(double) * static_cast<size_t>(pl->n_tiles) * n_p));
  TRY(ensure(ctx, ctx->lik_partial_cnt, sizeof(unsigned) * static_cast<size_t>(pl->n_tiles) * n_p));
  if (strict)
  {
    TRY(ensure(ctx, ctx->strict_terms, strict_plan_bytes(ctx, n_p, ns, pl->group_size)));
    pl->strict_terms = ctx->strict_terms.as<float>();
    pl->chunk = (ctx->scan_chunk && static_cast<size_t>(ns) > ctx->scan_chunk) ? ctx->scan_chunk : 0;
    if (pl->chunk)
      TRY(ensure_replay_stream(ctx));
  }
  return 0;
}

// size check and buffers of a beam launch of n_p particles x n_b > 0 points (statistics and production path alike)
int prepare_beam(mcl3dl_hip_ctx* ctx, size_t n_p, long long* n_rays, long long* blocks)
{
  TRY(ensure_pow_table(ctx));
  *n_rays = static_cast<long long>(n_p) * static_cast<long long>(ctx->n_b);
  *blocks = (*n_rays + 255) / 256;
  if (*blocks > 0x7fffffffLL)
    return ctx->fail(-3, "too many rays for one launch");
  const size_t cap0 = ctx->penalty.cap;
  TRY(ensure(ctx, ctx->penalty, sizeof(unsigned) * n_p));
  if (ctx->penalty.cap != cap0)
    ctx->penalty_clean_n = 0;  // (a new allocation: nothing is known about its content)
  return 0;
}

// the beam side of the plan; with_lik: a likelihood kernel runs in this call (pl holds its plan already)
int plan_beam(mcl3dl_hip_ctx* ctx, size_t n_p, bool with_lik, MeasurePlan* pl)
{
  if (ctx->n_b == 0)
  {
    // (1, 0) for every particle; with the tiled likelihood kernel behind it the per-particle finalize writes the ones
    pl->beam = with_lik && pl->tiled() ? BeamRoute::OnesByFinalize : BeamRoute::OnesByFill;
    return 0;
  }
  TRY(prepare_beam(ctx, n_p, &pl->n_rays, &pl->beam_blocks));
  const long long n_rays = pl->n_rays, blocks = pl->beam_blocks;
  // (the prepared origins and the launches of both models below are the DDA walk's: the kd-tree caster runs as a launch of
  // its own, behind or — from OVERLAP_MIN_RAYS rays — beside the likelihood kernel on the second stream)
  pl->kd = ctx->beam_raycast == 1;
  pl->prepared = !pl->kd && ctx->opt.beam_prepare && n_rays >= BEAM_PREPARE_MIN_RAYS &&
                 static_cast<long long>(n_p) * static_cast<long long>(ctx->n_o) < 0x7fffffffLL;
  if (pl->prepared)
    TRY(ensure(ctx, ctx->beam_origin, sizeof(BeamOrigin) * n_p * ctx->n_o));
  // Both models in ONE launch (lik_beam_kernel, update_kernels.h: the two kernels' work-groups interleaved, so that every CU
  // hosts both all the way) whenever the likelihood side is the tiled kernel's cooperative fp64-tree form (G <= 16) and the beam side is large
  // enough to be worth interleaving: the beam kernel is NOT launched on its own but with the tiled kernel.
  // Not in front of a LONG caller-order replay (replay_is_long below): on two streams that replay — memory-bound, VALU idle —
  // overlaps the rest of the beam kernel, which the lock-step interleave cannot offer (C5 shard: 3.09 against 3.14 ms).
  // Measured, C3: 0.3446 (two streams) -> 0.3313 ms; 4096 rays per particle: 1.0855 -> 1.0070 (profiles/r06s_lik_beam_one_launch.txt).
  // (the beam kernel's map-update-overlay form needs 66 VGPRs: it would spill inside the 64 of the merged launch)
  const bool mergeable = !pl->kd && ctx->opt.overlap_models && with_lik && ctx->dg.ov_n == 0;
  const bool with_tiled = mergeable && pl->group_size <= 16 && pl->coop && blocks >= 64 && blocks < 0x3fffffffLL &&
                          pl->blocks < 0x3fffffffLL;
  // (in front of the caller-order replay: two streams only where they would be used — from OVERLAP_MIN_RAYS rays — AND the replay
  // is long enough to hide the beam kernel's tail behind: a term array of at least half a gigabyte. Measured, merged against
  // streams: 4096 x 4096 + 128 rays - 12 %, 16384 x 4096 + 512 (268 MB) - 3 %, 8192 x 32768 + 512 (1 GB) + 1 %, the C5 shard + 2 %:
  // profiles/r06s_lik_beam_one_launch.txt)
  pl->replay_is_long = pl->strict_terms != nullptr && n_rays >= OVERLAP_MIN_RAYS &&
                       strict_terms_bytes(n_p, static_cast<int>(ctx->n_s), pl->group_size) >= (static_cast<size_t>(512) << 20);
  if (with_tiled && pl->lik == LikRoute::Tiled && !pl->chunk && !pl->replay_is_long)
    pl->beam = BeamRoute::MergedTiled;
  // (the in-kernel chain's single-tile form, strict_order 3, rides the same way: a consumer's producer keeps its lower block index)
  else if (with_tiled && pl->lik == LikRoute::Chain)
    pl->beam = BeamRoute::MergedChain;
  // (the per-particle likelihood kernel's 64- and 256-thread forms take the beam kernel's work-groups along the same way:
  // lik_particle_beam_kernel)
  else if (mergeable && pl->lik == LikRoute::Particle && ctx->opt.lik_index == 2 && pl->block != 1024 && blocks >= 16 && blocks < 0x0fffffffLL)
    pl->beam = BeamRoute::MergedParticle;
  // the second stream pays only for large launches: the fork / join events cost ~35 us (64 particles x 96 + 3 points:
  // 52 us per update with them, 17 without), the overlap itself is worth ~5 % at C3 (2.1 M rays)
  else if (ctx->opt.overlap_models && with_lik && n_rays >= OVERLAP_MIN_RAYS)
    pl->beam = BeamRoute::Aux;
  else
    pl->beam = BeamRoute::Main;
  return 0;
}

// The plan of one call (the map structures are in place: lik_defer_active, ctx->dg.ov_n and ctx->rg are valid).
int plan_measure(mcl3dl_hip_ctx* ctx, size_t n_p, bool want_lik, bool have_lik_out, bool want_beam, MeasurePlan* pl)
{
  if (want_lik)
  {
    pl->lik = LikRoute::Ones;
    if (ctx->n_s > 0)
      TRY(plan_lik(ctx, n_p, static_cast<int>(ctx->n_s), pl));
    ctx->lik_exact = pl->lik_exact = ctx->n_s == 0 || pl->rows || pl->chain() || pl->strict_terms != nullptr;
  }
  if (want_beam)
    TRY(plan_beam(ctx, n_p, want_lik && ctx->n_s > 0, pl));
  if (pl->chain() && !have_lik_out)  // (only the match ratio was asked for: the chain's sum still has somewhere to go)
    TRY(ensure(ctx, ctx->chain_lik, sizeof(float) * n_p));
  return 0;
}

// ---- the launchers: one per route ---------------------------------------------------------------------------------------
// What launch_measure leaves to the kernel behind it when the caller asks for it (`want`: the split pf::measure follows on the
// same stream): the sum over the tiled kernel's per-tile partials — d_lik / d_ratio (and d_beam's ones, `beam_fill`) are then NOT
// written by launch_measure but by lik_pf_partial_kernel (pf_kernels.h: LikTiles), one launch less per update.
struct LikTail
{
  bool want = false;
  bool pending = false, beam_fill = false;
  int n_tiles = 0;
  // the beam model's last step (penalty count -> score, beam_finalize_kernel) left to that kernel as well: ctx->penalty holds the
  // counts, d_beam is NOT written yet (pf_one_gpu runs beam_finalize_kernel itself when its kernel cannot take the counts)
  bool want_beam = false, beam_pending = false;
};

// one launch_measure call as its launchers see it
struct MeasureCall
{
  mcl3dl_hip_ctx* ctx;
  const MeasurePlan& plan;
  const float* d_pose;
  size_t n_p;
  int np;
  float *d_lik, *d_ratio, *d_beam;
  LikTail* tail;
  LikParams lp;
  const float4* scan;
  int ns;

  // d_beam where whatever finishes the tiled kernel's sums also writes the beam model's ones
  float* beam_ones() const
  {
    return plan.beam == BeamRoute::OnesByFinalize ? d_beam : nullptr;
  }
};

// any return between the fork and the join of launch_measure (a failing HIP call) first waits for the second stream, so the
// caller never gets control back with beam kernels still writing its buffers
struct ForkGuard
{
  mcl3dl_hip_ctx* c;
  bool armed = false;
  ~ForkGuard()
  {
    if (armed)
      (void)hipStreamSynchronize(c->aux_stream);
  }
};

// the beam model's last step (penalty counts -> scores): left to the update's tail kernel, or a launch of its own
void finish_beam(const MeasureCall& c, hipStream_t on)
{
  const mcl3dl_hip_ctx* ctx = c.ctx;
  if (c.tail && c.tail->want_beam)
    c.tail->beam_pending = true;
  else
    hipLaunchKernelGGL(beam_finalize_kernel, dim3((c.np + 255) / 256), dim3(256), 0, on, ctx->penalty.as<unsigned>(),
                       ctx->pow_table.as<float>(), ctx->beam_likelihood_min, c.d_beam, c.np);
}

// the penalty counters of np particles to zero on stream `on`
void zero_penalty(mcl3dl_hip_ctx* ctx, int np, hipStream_t on)
{
  // a kernel, not hipMemsetAsync: a memset node at the head of a single-stream captured update faulted on its third
  // replay (ROCm 7.2; 700 particles x 3 rays, 128 x 48), the same zeroing as a kernel node does not
  hipLaunchKernelGGL(fill_kernel, dim3((np + 255) / 256), dim3(256), 0, on, reinterpret_cast<float*>(ctx->penalty.p), 0.0f,
                     static_cast<float*>(nullptr), 0.0f, np);
}

// The beam model: its ones, or — on the main or the second stream — counter zeroing, origin preparation, the caster and the
// last step; with a merged route the rays ride in the likelihood kernel's launch, which also takes the last step behind itself.
int launch_beam(const MeasureCall& c, ForkGuard* fork_guard)
{
  mcl3dl_hip_ctx* ctx = c.ctx;
  const MeasurePlan& pl = c.plan;
  if (pl.beam == BeamRoute::OnesByFinalize)
    return 0;
  if (pl.beam == BeamRoute::OnesByFill)
  {
    hipLaunchKernelGGL(fill_kernel, dim3((c.np + 255) / 256), dim3(256), 0, ctx->stream, c.d_beam, 1.0f,
                       static_cast<float*>(nullptr), 0.0f, c.np);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  const bool overlap = pl.beam == BeamRoute::Aux;
  hipStream_t bs = overlap ? ctx->aux_stream : ctx->stream;
  if (overlap)
  {
    HIP_TRY(hipEventRecord(ctx->ev_fork, ctx->stream));
    HIP_TRY(hipStreamWaitEvent(bs, ctx->ev_fork, 0));
    fork_guard->armed = true;
  }
  EventPair ep{};
  TRY(timing_begin(ctx, MCL3DL_KERNEL_BEAM, &ep, bs));
  // (beam_origin_kernel zeroes the counters itself; the update's tail kernel leaves them zeroed behind itself)
  const bool counters_clean = ctx->penalty_clean_n >= c.n_p;
  ctx->penalty_clean_n = 0;  // ... and from here on they are in use
  if (!pl.prepared && !counters_clean)
    zero_penalty(ctx, c.np, bs);
  // what depends only on (particle, origin) is computed once per pair when the launch is large enough to pay for
  // one more kernel
  const BeamOrigin* prepared = nullptr;
  if (pl.prepared)
  {
    const long long n_pairs = static_cast<long long>(c.n_p) * static_cast<long long>(ctx->n_o);
    hipLaunchKernelGGL(beam_origin_kernel, dim3(static_cast<unsigned>((n_pairs + 255) / 256)), dim3(256), 0, bs, c.d_pose,
                       c.np, ctx->origins.as<float4>(), static_cast<int>(ctx->n_o), ctx->dg,
                       ctx->beam_origin.as<BeamOrigin>(), ctx->penalty.as<unsigned>());
    prepared = ctx->beam_origin.as<BeamOrigin>();
  }
  if (pl.beam == BeamRoute::Main || pl.beam == BeamRoute::Aux)  // (merged: the rays ride in the likelihood kernel's launch)
  {
    const dim3 grid(static_cast<unsigned>(pl.beam_blocks));
    if (pl.kd)
      hipLaunchKernelGGL(beam_kd_kernel, grid, dim3(256), 0, bs, c.d_pose, ctx->scan_beam.as<float4>(),
                         static_cast<int>(ctx->n_b), ctx->origins.as<float4>(), pl.n_rays, ctx->lg, kd_ray_params(ctx),
                         beam_params(ctx), ctx->penalty.as<unsigned>());
    else
    {
      // (a map update rides on the DDA grid as an overlay: the kernel that looks it up is chosen only then)
      const auto kernel = ctx->dg.ov_n > 0 ? beam_kernel<false, true> : beam_kernel<false, false>;
      hipLaunchKernelGGL(kernel, grid, dim3(256), 0, bs, c.d_pose, ctx->scan_beam.as<float4>(), static_cast<int>(ctx->n_b),
                         ctx->origins.as<float4>(), pl.n_rays, ctx->dg, beam_params(ctx), ctx->penalty.as<unsigned>(),
                         static_cast<RayStats*>(nullptr), prepared, static_cast<int>(ctx->n_o));
    }
    finish_beam(c, bs);
  }
  TRY(timing_end(ctx, ep, bs));
  if (overlap)
    HIP_TRY(hipEventRecord(ctx->ev_join, bs));
  HIP_TRY(hipGetLastError());
  return 0;
}

// What a launch of both models has in common: the poses, the likelihood model's grids and the beam side with the interleave
// of n_beam beam work-groups with n_other of the likelihood kernel's (LikBeamArgs / LikParticleBeamArgs).
template <class Args>
Interleave merged_args(const MeasureCall& c, long long n_beam, long long n_other, Args* a)
{
  mcl3dl_hip_ctx* ctx = c.ctx;
  const Interleave il = interleave(n_beam, n_other);
  a->pose7 = c.d_pose;
  a->n_p = c.np;
  a->g = ctx->lg;
  a->rg = tiled_rec_grid(ctx, c.lp);  // (the per-particle kernels ignore common_map)
  a->prm = c.lp;
  a->scan_beam = ctx->scan_beam.as<float4>();
  a->n_b = static_cast<int>(ctx->n_b);
  a->origins = ctx->origins.as<float4>();
  a->n_rays = c.plan.n_rays;
  a->dg = ctx->dg;
  a->bp = beam_params(ctx);
  a->penalty = ctx->penalty.as<unsigned>();
  a->prepared = c.plan.prepared ? ctx->beam_origin.as<BeamOrigin>() : nullptr;
  a->n_o = static_cast<int>(ctx->n_o);
  a->beam8 = il.beam8;
  a->n_beam_blocks = static_cast<uint32_t>(n_beam);
  return il;
}

// lik_beam_kernel<G, DEFER, false, CHAIN>: the tiled kernel over n_s points from `scan` (t_blocks work-groups) with the beam
// kernel's work-groups in between, and the beam model's last step behind it. The caller sets a's partials / terms / chain.
template <bool CHAIN>
void launch_lik_beam(const MeasureCall& c, long long t_blocks, const float4* scan, int n_s, int n_tiles, LikBeamArgs& a)
{
  mcl3dl_hip_ctx* ctx = c.ctx;
  const Interleave il = merged_args(c, c.plan.beam_blocks, t_blocks, &a);
  a.n_groups = c.plan.n_groups;
  a.strict_skew4 = STRICT_SKEW4;
  a.tiled8 = il.other8;
  a.n_tiled_blocks = static_cast<uint32_t>(t_blocks);
  a.scan = scan;
  a.n_s = n_s;
  a.n_tiles = n_tiles;
  dispatch_int<4, 8, 16>(c.plan.group_size, [&](auto g) {
    dispatch_int<1, 0>(c.plan.defer, [&](auto defer) {
      hipLaunchKernelGGL((lik_beam_kernel<decltype(g)::value, decltype(defer)::value != 0, false, CHAIN>),
                         dim3(static_cast<unsigned>(il.grid)), dim3(256), 0, ctx->stream, a);
    });
  });
  finish_beam(c, ctx->stream);
}

// f(MODE, COOP, DEFER) of the tiled kernel, as constants
template <class F>
void dispatch_form(const MeasurePlan& pl, F&& f)
{
  using Mode2 = std::integral_constant<int, 2>;
  if (pl.coop && pl.defer)
    f(Mode2{}, std::true_type{}, std::true_type{});
  else if (pl.coop)
    f(Mode2{}, std::true_type{}, std::false_type{});
  else if (pl.mode == 2)
    f(Mode2{}, std::false_type{}, std::false_type{});
  else
    f(std::integral_constant<int, 0>{}, std::false_type{}, std::false_type{});
}

void launch_small(const MeasureCall& c)
{
  mcl3dl_hip_ctx* ctx = c.ctx;
  const MeasurePlan& pl = c.plan;
  const uint32_t* row_perm = pl.rows ? ctx->scan_perm.as<uint32_t>() : nullptr;
  dispatch_int<1, 2, 4, 8, 16, 32>(pl.W, [&](auto w) {
    dispatch_int<2, 0>(pl.mode, [&](auto m) {
      hipLaunchKernelGGL((likelihood_small_kernel<decltype(w)::value, decltype(m)::value>), dim3(static_cast<unsigned>(pl.blocks)),
                         dim3(256), 0, ctx->stream, c.d_pose, c.np, c.scan, c.ns, ctx->lg, ctx->rg, c.lp, c.d_lik, c.d_ratio,
                         pl.coop ? 1 : 0, row_perm);
    });
  });
}

// one launch of the tiled kernel over t_ns points starting at t_scan (the whole scan, or one chunk of it), alone or with
// the beam kernel's work-groups
void launch_tiled(const MeasureCall& c, const float4* t_scan, int t_ns, int t_tiles, double* t_psum, unsigned* t_pcnt,
                  const uint32_t* t_perm, float* t_terms)
{
  mcl3dl_hip_ctx* ctx = c.ctx;
  const MeasurePlan& pl = c.plan;
  const long long t_blocks = tiled_blocks(t_tiles, pl.n_groups);
  if (pl.beam == BeamRoute::MergedTiled)
  {
    LikBeamArgs a{};
    a.partial_sum = t_psum;
    a.partial_cnt = t_pcnt;
    a.scan_perm = t_perm;
    a.strict_terms = t_terms;
    launch_lik_beam<false>(c, t_blocks, t_scan, t_ns, t_tiles, a);
    return;
  }
  dispatch_int<4, 8, 32, 16>(pl.group_size, [&](auto g) {
    dispatch_form(pl, [&](auto mode, auto coop, auto defer) {
      constexpr int G = decltype(g)::value;
      constexpr int MINW = G == 32 ? 4 : 8;  // G = 32: 33 KB of LDS per work-group, 4 wavefronts per SIMD at most
      hipLaunchKernelGGL((likelihood_tiled_kernel<G, decltype(mode)::value, MINW, decltype(coop)::value, decltype(defer)::value>), dim3(static_cast<unsigned>(t_blocks)),
                         dim3(256), 0, ctx->stream, c.d_pose, c.np, t_scan, t_ns, t_tiles, pl.n_groups, ctx->lg, tiled_rec_grid(ctx, c.lp),
                         c.lp, t_psum, t_pcnt, t_perm, t_terms, STRICT_SKEW4);
    });
  });
}

// lik_strict_sum_rows_kernel with as many particle groups per work-group as keep the launch in ONE round of work-groups, up to a
// full adder wavefront (64 lanes / GG particles per group)
template <int GG>
void launch_strict_sum(mcl3dl_hip_ctx* ctx, const float* strict_terms, int ns, int np, int n_groups, float* d_lik, hipStream_t on,
                       int accumulate)
{
  constexpr int MAX_GPW = 64 / GG >= 4 ? 4 : (64 / GG >= 2 ? 2 : 1);
  int gpw = n_groups <= ctx->n_cus ? 1 : (n_groups <= 2 * ctx->n_cus ? 2 : 4);
  gpw = std::min(gpw, MAX_GPW);
  const auto launch = [&](auto chunk, auto per_wg) {
    constexpr int GPW = decltype(per_wg)::value;
    hipLaunchKernelGGL((lik_strict_sum_rows_kernel<GG, decltype(chunk)::value, GPW>), dim3((n_groups + GPW - 1) / GPW), dim3(1024),
                       0, on, strict_terms, ns, np, n_groups, d_lik, STRICT_SKEW4, accumulate);
  };
  using std::integral_constant;
  if constexpr (MAX_GPW >= 4)
    if (gpw == 4)
      return launch(integral_constant<int, 16384>{}, integral_constant<int, 4>{});
  if constexpr (MAX_GPW >= 2)
    if (gpw >= 2)
      return launch(integral_constant<int, 32768>{}, integral_constant<int, 2>{});
  launch(integral_constant<int, 65536>{}, integral_constant<int, 1>{});
}

// the float-order replay of r_ns points' terms into d_lik (accumulate: continued from the sums already there)
void launch_replay(const MeasureCall& c, const float* terms, int r_ns, hipStream_t on, int accumulate)
{
  dispatch_int<4, 8, 32, 16>(c.plan.group_size, [&](auto g) {
    launch_strict_sum<decltype(g)::value>(c.ctx, terms, r_ns, c.np, c.plan.n_groups, c.d_lik, on, accumulate);
  });
}

// The tiled kernel over the whole scan, then whatever adds its tiles up: the caller's tail kernel, lik_finalize_kernel, and the
// float-order replay of the term array.
void launch_tiled_scan(const MeasureCall& c)
{
  mcl3dl_hip_ctx* ctx = c.ctx;
  const MeasurePlan& pl = c.plan;
  double* const psum = ctx->lik_partial_sum.as<double>();
  unsigned* const pcnt = ctx->lik_partial_cnt.as<unsigned>();
  // (a chunk-ordered scan whose likelihoods nobody asked for: its permutation is chunk-relative, no terms are kept)
  launch_tiled(c, c.scan, c.ns, pl.n_tiles, psum, pcnt, ctx->scan_perm.as<uint32_t>(), pl.chunk ? nullptr : pl.strict_terms);
  if (c.tail && c.tail->want && !pl.strict_terms && c.d_lik && c.d_ratio)
  {
    c.tail->pending = true;  // lik_pf_partial_kernel adds the tiles up
    c.tail->n_tiles = pl.n_tiles;
    c.tail->beam_fill = pl.beam == BeamRoute::OnesByFinalize;
  }
  else
    hipLaunchKernelGGL(lik_finalize_kernel, dim3((c.np + 31) / 32), dim3(256), 0, ctx->stream, psum, pcnt, pl.n_tiles, c.np, c.ns,
                       c.d_lik, c.d_ratio, c.beam_ones());
  if (pl.strict_terms && c.d_lik && !pl.chunk)
    launch_replay(c, pl.strict_terms, c.ns, ctx->stream, 0);
}

// The scan was ordered in chunks of the caller's order (host_cloud.h:device_order_scans). Chunk c is evaluated on the
// context's stream into term buffer c % 2 while chunk c - 1 is replayed — the reference's float recurrence continued
// from the sums chunk c - 2 ... left in d_lik — on a stream of its own: the replay streams its terms at memory speed,
// the evaluation is bound by VALU issue, and the two share the GPU well; the buffer holds two chunks, not the scan.
int launch_chunked_replay(const MeasureCall& c)
{
  mcl3dl_hip_ctx* ctx = c.ctx;
  const MeasurePlan& pl = c.plan;
  const size_t chunk = pl.chunk, n_p = c.n_p;
  const int ns = c.ns, np = c.np;
  const int n_chunks = static_cast<int>((static_cast<size_t>(ns) + chunk - 1) / chunk);
  double* const psum = ctx->lik_partial_sum.as<double>();
  unsigned* const pcnt = ctx->lik_partial_cnt.as<unsigned>();
  float* const buf[2] = { pl.strict_terms,
                          pl.strict_terms + strict_terms_bytes(n_p, static_cast<int>(chunk), pl.group_size) / sizeof(float) };
  bool failed = false;
  for (int k = 0; k < n_chunks && !failed; ++k)
  {
    const size_t first = static_cast<size_t>(k) * chunk;
    const int c_ns = static_cast<int>(std::min(chunk, static_cast<size_t>(ns) - first));
    const int c_tiles = (c_ns + 255) / 256, tile0 = static_cast<int>(first / 256);
    if (k >= 2)
      failed = failed || hipStreamWaitEvent(ctx->stream, ctx->ev_replay[k & 1], 0) != hipSuccess;  // its buffer is free again
    launch_tiled(c, c.scan + first, c_ns, c_tiles, psum + static_cast<size_t>(tile0) * n_p, pcnt + static_cast<size_t>(tile0) * n_p,
                 ctx->scan_perm.as<uint32_t>() + first, buf[k & 1]);
    failed = failed || hipEventRecord(ctx->ev_tiled[k & 1], ctx->stream) != hipSuccess ||
             hipStreamWaitEvent(ctx->replay_stream, ctx->ev_tiled[k & 1], 0) != hipSuccess;
    launch_replay(c, buf[k & 1], c_ns, ctx->replay_stream, k > 0 ? 1 : 0);
    failed = failed || hipEventRecord(ctx->ev_replay[k & 1], ctx->replay_stream) != hipSuccess;
  }
  // match ratios (and nothing else: the likelihoods are the replay's) from the per-tile counts
  hipLaunchKernelGGL(lik_finalize_kernel, dim3((np + 31) / 32), dim3(256), 0, ctx->stream, psum, pcnt, pl.n_tiles, np, ns,
                     static_cast<float*>(nullptr), c.d_ratio, c.beam_ones());
  if (failed || hipStreamWaitEvent(ctx->stream, ctx->ev_replay[(n_chunks - 1) & 1], 0) != hipSuccess)
  {
    const int r = ctx->fail(-2, "stream / event call failed in the chunked float-order replay: %s", hipGetErrorString(hipGetLastError()));
    (void)hipStreamSynchronize(ctx->replay_stream);  // (nothing of the replay is still in flight when the caller hears of it)
    return r;
  }
  return 0;
}

// strict_order 3: the chain forms of the tiled kernel, one launch of one device at a time (ChainSerial)
int launch_chain(const MeasureCall& c)
{
  mcl3dl_hip_ctx* ctx = c.ctx;
  const MeasurePlan& pl = c.plan;
  ChainSerial& cs = chain_serial(ctx->device);
  std::lock_guard<std::mutex> chain_lock(cs.m);
  if (cs.ev)
    HIP_TRY(hipStreamWaitEvent(ctx->stream, cs.ev, 0));
  else
    HIP_TRY(hipEventCreateWithFlags(&cs.ev, hipEventDisableTiming));
  struct ChainDone  // (recorded behind the launch on every way out of this function)
  {
    hipEvent_t ev;
    hipStream_t st;
    ~ChainDone()
    {
      (void)hipEventRecord(ev, st);
    }
  } chain_done{ cs.ev, ctx->stream };
  // (only the match ratio was asked for: the sum still has somewhere to go)
  float* const lik_out = c.d_lik ? c.d_lik : ctx->chain_lik.as<float>();
  const LikChain lc{ ctx->chain_carry.as<unsigned long long>(), pl.chain_tag0, lik_out, c.d_ratio, c.beam_ones(), ctx->chain_err };
  const dim3 grid(static_cast<unsigned>(pl.blocks));
  if (pl.lik == LikRoute::ChainMulti)
    hipLaunchKernelGGL((likelihood_chain_multi_kernel<4, 4>), grid, dim3(256), 0, ctx->stream, c.d_pose, c.np, c.scan, c.ns,
                       pl.n_tiles, pl.n_super, pl.n_groups, ctx->rg, c.lp, lc);
  else if (pl.beam == BeamRoute::MergedChain)
  {
    LikBeamArgs a{};
    a.ch = lc;
    launch_lik_beam<true>(c, pl.blocks, c.scan, c.ns, pl.n_tiles, a);
  }
  else
    dispatch_int<4, 8, 16>(pl.group_size, [&](auto g) {
      dispatch_form(pl, [&](auto mode, auto coop, auto defer) {
        hipLaunchKernelGGL((likelihood_tiled_kernel<decltype(g)::value, decltype(mode)::value, 8, decltype(coop)::value, decltype(defer)::value, true>),
                           grid, dim3(256), 0, ctx->stream, c.d_pose, c.np, c.scan, c.ns, pl.n_tiles, pl.n_groups, ctx->lg,
                           tiled_rec_grid(ctx, c.lp), c.lp,
                           static_cast<double*>(nullptr), static_cast<unsigned*>(nullptr), static_cast<const uint32_t*>(nullptr),
                           static_cast<float*>(nullptr), 0, lc);
      });
    });
  return 0;
}

// the per-particle kernel, alone or with the beam kernel's work-groups (rays per beam work-group = its work-group size)
void launch_particle(const MeasureCall& c)
{
  mcl3dl_hip_ctx* ctx = c.ctx;
  const MeasurePlan& pl = c.plan;
  // caller-order float sums inside the kernel: the permutation (device index -> caller's index) and the LDS row of
  // chain_row_floats(ns) floats
  const uint32_t* row_perm = pl.rows ? ctx->scan_perm.as<uint32_t>() : nullptr;
  const size_t row_bytes = pl.rows ? sizeof(float) * static_cast<size_t>(chain_row_floats(c.ns)) : 0;
  if (pl.beam == BeamRoute::MergedParticle)
  {
    LikParticleBeamArgs a{};
    const Interleave il = merged_args(c, (pl.n_rays + pl.block - 1) / pl.block, c.np, &a);
    a.scan = c.scan;
    a.n_s = c.ns;
    a.out_lik = c.d_lik;
    a.out_ratio = c.d_ratio;
    a.coop = pl.coop ? 1 : 0;
    a.perm = row_perm;
    a.lik8 = il.other8;
    dispatch_int<64, 256>(pl.block, [&](auto b) {
      constexpr int BLOCK = decltype(b)::value;
      hipLaunchKernelGGL(lik_particle_beam_kernel<BLOCK>, dim3(static_cast<unsigned>(il.grid)), dim3(BLOCK), row_bytes, ctx->stream, a);
    });
    finish_beam(c, ctx->stream);
    return;
  }
  dispatch_particle(pl.block, pl.mode, [&](auto b, auto m) {
    constexpr int BLOCK = decltype(b)::value;
    hipLaunchKernelGGL((likelihood_kernel<BLOCK, decltype(m)::value, false>), dim3(c.np), dim3(BLOCK), row_bytes, ctx->stream, c.d_pose,
                       c.scan, c.ns, ctx->lg, ctx->rg, c.lp, c.d_lik, c.d_ratio, nullptr, pl.coop ? 1 : 0, row_perm);
  });
}

int launch_lik(const MeasureCall& c)
{
  mcl3dl_hip_ctx* ctx = c.ctx;
  const MeasurePlan& pl = c.plan;
  if (pl.lik == LikRoute::Ones)
  {
    hipLaunchKernelGGL(fill_kernel, dim3((c.np + 255) / 256), dim3(256), 0, ctx->stream, c.d_lik, 1.0f, c.d_ratio, 0.0f, c.np);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  EventPair ep{};
  TRY(timing_begin(ctx, MCL3DL_KERNEL_LIKELIHOOD, &ep));
  if (pl.lik == LikRoute::Small)
    launch_small(c);
  else if (pl.chain())
    TRY(launch_chain(c));
  else if (pl.lik == LikRoute::Tiled && pl.strict_terms && pl.chunk && c.d_lik)
    TRY(launch_chunked_replay(c));
  else if (pl.lik == LikRoute::Tiled)
    launch_tiled_scan(c);
  else
    launch_particle(c);
  TRY(timing_end(ctx, ep));
  HIP_TRY(hipGetLastError());
  return 0;
}

// One scan update's likelihoods, match ratios and beam scores of n_p poses (each output may be null): ensure the map
// structures, plan, enqueue the beam model, enqueue the likelihood-field model, join.
int launch_measure(mcl3dl_hip_ctx* ctx, const float* d_pose, size_t n_p, float* d_lik, float* d_ratio, float* d_beam,
                   LikTail* tail = nullptr)
{
  if (!ctx->has_scan)
    return ctx->fail(-5, "no scan uploaded: call mcl3dl_hip_upload_scan first");
  if (n_p == 0)
    return 0;
  if (n_p > 0x7fffffffu)
    return ctx->fail(-3, "too many particles");
  const bool want_lik = d_lik || d_ratio, want_beam = d_beam != nullptr;
  TRY(ensure_caster_structures(ctx, want_lik && ctx->n_s > 0, want_beam && ctx->n_b > 0));
  MeasurePlan plan;
  TRY(plan_measure(ctx, n_p, want_lik, d_lik != nullptr, want_beam, &plan));
  const MeasureCall c{ ctx,  plan, d_pose, n_p, static_cast<int>(n_p), d_lik, d_ratio, d_beam, tail, lik_params(ctx),
                       ctx->scan_lik.as<float4>(), static_cast<int>(ctx->n_s) };
  ForkGuard fork_guard{ ctx };
  // (the beam model is enqueued first: on its own stream when both models run, see mcl3dl_hip_ctx::aux_stream)
  if (want_beam)
    TRY(launch_beam(c, &fork_guard));
  if (want_lik)
    TRY(launch_lik(c));
  if (fork_guard.armed)
  {
    HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));  // later work on `stream` sees the beam scores
    fork_guard.armed = false;
  }
  return 0;
}

// mcl3dl_hip_workload_stats: the work one update does — candidates tested by the likelihood model, steps / occupied cells /
// tests of the beam model's DDA walk (the ray statistics are that walk's: this path stays on the DDA caster whatever
// beam_raycast says) — counted by instrumented kernels; no result array is written.
int measure_stats(mcl3dl_hip_ctx* ctx, const float* d_pose, size_t n_p, double* stats6)
{
  if (!ctx->has_scan)
    return ctx->fail(-5, "no scan uploaded: call mcl3dl_hip_upload_scan first");
  if (n_p == 0)
    return 0;
  if (n_p > 0x7fffffffu)
    return ctx->fail(-3, "too many particles");
  TRY(ensure_structures(ctx, ctx->n_s > 0, ctx->n_b > 0, true));
  const int np = static_cast<int>(n_p);
  if (ctx->n_s > 0)
    TRY(ensure(ctx, ctx->tested, sizeof(double) * n_p));
  if (ctx->n_b > 0)
  {
    long long n_rays = 0, blocks = 0;
    TRY(prepare_beam(ctx, n_p, &n_rays, &blocks));
    TRY(ensure(ctx, ctx->ray_stats, sizeof(RayStats)));
    const bool counters_clean = ctx->penalty_clean_n >= n_p;
    ctx->penalty_clean_n = 0;
    if (!counters_clean)
      zero_penalty(ctx, np, ctx->stream);
    HIP_TRY(hipMemsetAsync(ctx->ray_stats.p, 0, sizeof(RayStats), ctx->stream));
    hipLaunchKernelGGL((beam_kernel<true>), dim3(static_cast<unsigned>(blocks)), dim3(256), 0, ctx->stream, d_pose,
                       ctx->scan_beam.as<float4>(), static_cast<int>(ctx->n_b), ctx->origins.as<float4>(), n_rays, ctx->dg,
                       beam_params(ctx), ctx->penalty.as<unsigned>(), ctx->ray_stats.as<RayStats>(),
                       static_cast<const BeamOrigin*>(nullptr), static_cast<int>(ctx->n_o));
  }
  HIP_TRY(hipGetLastError());
  if (ctx->n_s > 0)
    hipLaunchKernelGGL((likelihood_kernel<256, 0, true>), dim3(np), dim3(256), 0, ctx->stream, d_pose, ctx->scan_lik.as<float4>(),
                       static_cast<int>(ctx->n_s), ctx->lg, ctx->rg, lik_params(ctx), nullptr, nullptr, ctx->tested.as<double>(), 0);
  HIP_TRY(hipGetLastError());
  std::vector<double> tested(ctx->n_s ? n_p : 0);
  RayStats rs{ 0, 0, 0 };
  if (ctx->n_s)
    TRY(d2h(ctx, tested.data(), ctx->tested.p, sizeof(double) * n_p));
  if (ctx->n_b)
    TRY(d2h(ctx, &rs, ctx->ray_stats.p, sizeof(RayStats)));
  TRY(sync_stream(ctx));
  stats6[0] = std::accumulate(tested.begin(), tested.end(), 0.0);
  stats6[1] = static_cast<double>(n_p) * static_cast<double>(ctx->n_s);
  stats6[2] = static_cast<double>(rs.steps);
  stats6[3] = static_cast<double>(rs.occupied);
  stats6[4] = static_cast<double>(rs.tested);
  stats6[5] = static_cast<double>(n_p) * static_cast<double>(ctx->n_b);
  return 0;
}

bool pf_float_order(const mcl3dl_hip_ctx* ctx, size_t n_p);  // host_pf.h

// The whole update — both models and pf::measure — as ONE launch (update_kernels.h) where the sizes are launch-bound:
// returns 1 when it was enqueued, 0 when this update is not eligible (the caller then runs the separate kernels), < 0 on
// error. Eligible: one GPU, per-particle likelihood kernel (not the tiled / small-scan forms), at most update_small_max
// particles and 256 beam points.
int launch_update_small(mcl3dl_hip_ctx* ctx, const float* d_pose, size_t n_p, float* d_weight, const float* d_extra,
                        float* d_lik, float* d_ratio, float* d_beam, float* d_stats4, const PfEmit* ho = nullptr)
{
  if (!ctx->opt.update_small || n_p == 0 || ctx->n_b > 256 || ctx->opt.strict_order == 3 || !ctx->has_scan || !d_lik || !d_ratio || !d_beam)
    return 0;
  if (n_p > static_cast<size_t>(ctx->opt.update_small_max))
    return 0;
  if (ctx->beam_raycast == 1 && ctx->n_b > 0)
    return 0;  // the one-launch kernel casts with the DDA walk: the kd-tree caster runs through the separate kernels
  const int np = static_cast<int>(n_p), ns = static_cast<int>(ctx->n_s);
  // (decided without plan_lik's buffer allocations: the tiled form needs per-tile partials this path never touches)
  const LikMode mode = ns > 0 ? lik_mode(ctx, np, ns) : LikMode{};
  if (ns > 0 && (mode.tiled || lik_small_applies(ctx, mode, np, ns)))
    return 0;
  TRY(ensure_structures(ctx, ns > 0, ctx->n_b > 0));
  if (ctx->n_b > 0 && ctx->dg.ov_n > 0)
    return 0;  // a map update rides on the DDA grid: the one-launch kernel is compiled without the overlay lookup
  if (ctx->n_b > 0)
    TRY(ensure_pow_table(ctx));
  const int nvb = static_cast<int>((n_p + PF_BLOCK - 1) / PF_BLOCK);
  TRY(ensure(ctx, ctx->wnew, sizeof(float) * n_p));
  TRY(ensure(ctx, ctx->block_partials, sizeof(double) * 4 * static_cast<size_t>(nvb)));
  TRY(ensure(ctx, ctx->partial4, sizeof(double) * 4));
  const size_t n_tickets = static_cast<size_t>(nvb) * 37 + static_cast<size_t>(ticket_tree_size(nvb)) + 1;
  if (ctx->us_tickets.cap < sizeof(unsigned) * n_tickets)
  {
    TRY(ensure(ctx, ctx->us_tickets, sizeof(unsigned) * n_tickets));
    // (a kernel, not hipMemsetAsync: see zero_penalty — a memset node in a captured update faulted on replay)
    const int n_words = static_cast<int>(ctx->us_tickets.cap / sizeof(unsigned));
    hipLaunchKernelGGL(fill_kernel, dim3((n_words + 255) / 256), dim3(256), 0, ctx->stream,
                       reinterpret_cast<float*>(ctx->us_tickets.p), 0.0f, static_cast<float*>(nullptr), 0.0f,
                       n_words);  // the update kernel leaves them zero
  }
  UpdateSmallArgs a{};
  a.pose7 = d_pose;
  a.n_p = np;
  a.scan_lik = ctx->scan_lik.as<float4>();
  a.n_s = ns;
  a.g = ctx->lg;
  a.rg = ctx->rg;
  a.prm = lik_params(ctx);
  a.coop = lik_coop_active(ctx) ? 1 : 0;
  a.scan_beam = ctx->scan_beam.as<float4>();
  a.n_b = static_cast<int>(ctx->n_b);
  a.origins = ctx->origins.as<float4>();
  a.dg = ctx->dg;
  a.bp = beam_params(ctx);
  a.pow_table = ctx->pow_table.as<float>();
  a.w = d_weight;
  a.extra = d_extra;
  a.use_beam = 1;
  a.out_lik = d_lik;
  a.out_ratio = d_ratio;
  a.out_beam = d_beam;
  a.w_new = ctx->wnew.as<float>();
  a.vb_partials = ctx->block_partials.as<double>();
  a.tickets = ctx->us_tickets.as<unsigned>();
  a.packed = ctx->partial4.as<double>();
  a.stats4 = d_stats4;
  a.conformant = ctx->opt.update_small_conformant;
  a.emit = ho ? *ho : PfEmit{};
  // the reference's float recurrences, in its own order: the likelihood terms over the caller's scan (lik_particle's row) and —
  // where this launch also finishes pf::measure — the weights over the particles (pf.h:255-260)
  const bool rows = mode.rows, float_w = pf_float_order(ctx, n_p);
  a.perm = rows ? ctx->scan_perm.as<uint32_t>() : nullptr;
  a.float_order_w = float_w ? 1 : 0;
  ctx->lik_exact = rows || ns == 0;
  const size_t row_bytes = sizeof(float) * std::max<size_t>(rows ? chain_row_floats(ns) : 0, float_w ? chain_row_floats(np) : 0);
  EventPair ep{};
  TRY(timing_begin(ctx, MCL3DL_KERNEL_UPDATE, &ep));
  // (the separate likelihood kernel's work-group size, so that the lanes add in the same order)
  dispatch_particle(lik_particle_block(ctx, np, ns), ctx->opt.lik_index == 2 ? 2 : 0, [&](auto b, auto m) {
    constexpr int BLOCK = decltype(b)::value;
    hipLaunchKernelGGL((update_small_kernel<BLOCK, decltype(m)::value>), dim3(static_cast<unsigned>(n_p)), dim3(BLOCK), row_bytes,
                       ctx->stream, a);
  });
  TRY(timing_end(ctx, ep));
  HIP_TRY(hipGetLastError());
  return 1;
}

}  // namespace
