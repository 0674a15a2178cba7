// host_options.h — included by mcl3dl_hip.hip ahead of host_context.h, and on its own by tests/cpp/options_check.cpp (plain
// C++17, no HIP): what the CALLER sets (struct Options, the context's `opt`), described ONCE — kOptions, one row per key of
// mcl3dl_hip_set_option / _get_option with its field, value rule, error text and effects — and interpreted by option_set /
// option_get. What the engine resolves from it (index_budget_bytes, cand_aniso_active, cand_parts, scan_chunk, lik_exact, the dirty
// flags, the counters) is state and stays in the context. The thresholds nobody needs to move are the constants below.
#pragma once

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

// ---- thresholds that are constants (their setters went in round 6; each keeps the measurement it was set from) -----------
constexpr long long OVERLAP_MIN_RAYS = 262144;  // launches below this many rays keep both models on one stream
// up to this many particles a scan of > 512 points gets 1024 threads per particle: 512 x 16 wavefronts are ONE round of the
// chip's 8192 wavefront slots (profiles/r06m_wide_threshold.txt: 64 x 4096 27 -> 16 us, 300 x 3000 27 -> 22, 512 x 4096 34 -> 29;
// 1024 particles and more: 1.2 x SLOWER). Round 2 had set 64 from scans of ~1000 points; since round 6 this kernel serves
// every default-mode scan up to 4096 points below 2048 particles (caller-order rows)
constexpr int LIK_WIDE_MAX_PARTICLES = 512;
// pf::measure as ONE kernel up to this many particles (option pf_fused). Measured: one work-group beats three launches up to 1024
// particles, ties at 2048, loses at 4096
constexpr int PF_FUSED_MAX_PARTICLES = 1024;
// exact sums by the per-particle kernels' LDS rows below this many particles, by the tiled kernel + replay from it
constexpr int STRICT_ROWS_MAX_PARTICLES = 2048;
constexpr double POLL_QUERY_US = 5000.0;  // interval of the hipStreamQuery health checks while a completion wait naps
constexpr double LIK_DEFER_MIN_FRAC = 0.03;  // lik_defer 2: overflow rounds are deferred when more than this share of the voxels overflow
constexpr long long BEAM_PREPARE_MIN_RAYS = 32768;  // launches of at least this many rays take prepared ray constants (beam_prepare)
// strict_order = 3: the four-tile form up to this many particles (profiles/r05r_chain_multi.txt: slower from 2048)
constexpr int CHAIN_MULTI_MAX = 1536;

// `matched` of a likelihood evaluation follows from the radius test alone — every d2 < r2 gives dist = r - max(RN(sqrt(d2)), flat)
// >= 0 — when flat does not exceed r and the root of r2 = float(double(r) * r) rounds back to r: the root is monotone in d2, so
// RN(sqrt(d2)) <= RN(sqrt(r2)) = r. A NaN among the three fails a comparison. The tiled kernel's specialised pose loop then takes
// `matched` from the exec mask of its sqrt block instead of comparing dist with 0 (likelihood_kernels.h: eval_coop_first<true>);
// tests/cpp/match_exec_check.cpp walks every float d2 below r2.
inline bool lik_match_from_radius(float r, float r2, float flat)
{
  return flat <= r && sqrtf(r2) == r;
}

// ---- what the caller sets ------------------------------------------------------------------------------------------------
struct Options
{
  // The two LiDAR models are independent until pf::measure: 1 = the models of a large update run side by side (in one launch,
  // or the beam kernels on a second stream), 0 = behind each other
  int overlap_models = 1;
  // lik_index 2 = the candidate-voxel records (map_compiler.h) serve measure(), 0 = 27-cell scan of the cell grid (the canonical
  // structure of SURVEY.md 8d, also what STATS counts on)
  int lik_index = 2;
  int lik_small = 1;       // 1 = several particles share a wavefront when the scan has <= 32 points
  int lik_tiled = 1;       // 1 = tile-major XCD-aware kernel for large scans, 0 = one work-group per particle always
  int lik_tiled_min = 1024;  // scans of at least this many points take the tiled kernel
  int lik_group = 0;       // particles per work-group of the tiled kernel: 0 = chosen per launch, or 4 / 8 / 16 / 32
  int lik_coop = 1;        // tiled kernel: 1 = quad-cooperative record fetch + VALU-trimmed evaluation (same results)
  // tiled kernel with deferred overflow rounds: -1 = the pose loop specialised for the common map where the map and the
  // parameters allow it (host_measure.h:lik_tiled_fast_active), 0 = never. Same bits either way: a switch for A/B runs and for the
  // tests that hold one loop against the other, kept beside the table (api_support.inl:kSwitches), not a row of it
  int lik_tiled_fast = -1;
  int pf_fused = 1;        // 1 = pf::measure as ONE kernel up to PF_FUSED_MAX_PARTICLES particles on one GPU (same bits, two launches
                           // fewer)
  // 1 = add the likelihood terms AND the weights in the reference's float order (single GPU; bit-identical results);
  // 2 (default) = replay the likelihood terms in that order for scans of at least strict_auto_min points, where the
  // reference's own float rounding (a random walk of n_s roundings) reaches the 1e-5 tolerance of north_star; 0 = never
  int strict_order = 2;
  // strict_order 2: exact caller-order float sums for scans of at most strict_exact_max points and of at least strict_auto_min.
  // strict_auto_min comes from a bound, not from a measurement: the reference's float recurrence over n positive terms
  // differs from the exact sum by a random walk of n roundings, each within half an ulp of the running sum — relative
  // standard deviation <= 2^-24 sqrt(n) / 3 (ulp(s_i) <= 2^-23 s_i, s_i ~ (i / n) S) — while the fp64 tree is the exact sum
  // rounded once. Three standard deviations stay inside north_star's 1e-5 up to n = (1e-5 x 2^24)^2 = 28 147 points; from
  // there on the default replays the reference's own order. (A bound on the WORST case, n x 2^-24, would put that limit at
  // 168 points: sums of equal terms can drift systematically — which is what strict_exact_max and strict_order 1 are for.)
  int strict_auto_min = 28147;
  int strict_exact_max = 4096;
  double strict_auto_max_bytes = 0.0;  // > 0: the automatic replay is also skipped when its buffer would exceed this many bytes
  // strict_chunk > 0: a scan whose terms will be replayed in the caller's order is ORDERED in chunks of that order
  // (strict_chunk points each, Morton order inside a chunk; scan_perm then holds indices relative to the chunk): chunk c + 1 is
  // evaluated while chunk c is replayed on a stream of its own, and the term buffer holds two chunks instead of the whole scan
  // (host_measure.h). Measured and OFF by default (profiles/r05g_chunked_replay.txt): the term buffer of C5 shrinks from 17 GB to
  // 4.3 GB, but the update takes 27.9 instead of 25.6 ms — the replay's 1024-thread, 128 KB work-groups find no room next to
  // the tiled kernel's (eight 19 KB work-groups per CU), so the two do not overlap and the shorter launches cost their tails.
  int strict_chunk = 0;
  int scan_presorted = 0;  // likelihood scans arrive in the engine's order already — no ordering pass (see include/mcl3dl_hip.h)
  // the whole update as one launch (update_kernels.h) up to update_small_max particles when the per-particle likelihood
  // kernel would run anyway: same bits, two to four launches fewer. Measured (profiles/r03*_update_small.txt): ahead of the
  // separate kernels up to ~500 particles (64 x 96 + 3: 26.9 -> 22.4 us, 64 x 1000: 13.7 -> 10.3), behind from 1024 on —
  // every work-group's arrival is an atomic the memory side serialises, and there are as many as particles
  int update_small = 1;
  int update_small_max = 512;
  int update_small_conformant = 0;  // 1 = acq_rel arrival tickets at agent scope (update_kernels.h:last_arrival)
  // host-buffer updates (mcl3dl_hip_measure_update): update_stage = 1: the caller's scans / poses / weights are taken over by
  // ONE launch (stage_kernels.h:scan_stage_kernel — ordering included) for scans up to ST_MAX_POINTS points per model;
  // update_zero_copy = 1: that kernel reads them where they lie in page-locked host memory and the last kernel of the update
  // writes the results there (no DMA copy either way), 0 = one H2D copy of the staged block, one D2H copy of the results.
  // (Rounds 4-5 also carried a two-launch tail — pf_norm_kernel, every work-group recomputing the reduction — and a
  // per-particle-only form of the one-launch update; both measured slower than the split kernels and are gone: HISTORY.md.)
  int update_stage = 1;
  int update_zero_copy = 1;
  // host-buffer updates end by POLLING a word in page-locked memory that a one-thread kernel behind the update's last kernel
  // writes, instead of hipStreamSynchronize: 6.3 against 12.2 us for launch + completion of one kernel on this part
  // (profiles/r04e_launch_cost.txt). 2 (default) = every synchronisation of the context's stream is that word (scan
  // preparation -5..10 %, the post-update reductions -10 %, a whole filter iteration -8 %: profiles/r04ad_poll_all.txt),
  // 1 = only the host-buffer update and its relatives, 0 = hipStreamSynchronize everywhere.
  int poll_sync = 2;
  // completion waits: the polled word is spun on for at most poll_spin_us microseconds (covers every update up to a few
  // thousand particles), then polled between naps that grow with the time already waited (a 25 ms update of 65 536 particles
  // costs its caller ~2 ms of CPU, not 25), with hipStreamQuery looked at every few milliseconds so that a faulted queue
  // comes back as an error instead of an endless wait
  double poll_spin_us = 2000.0;
  bool test_late_structures = false;  // fault injection for the API-sequence fuzz (test hooks only)
  int cand_prune_coop = 1;  // 16 lanes per voxel in the map compiler's pruning pass (0 = one thread)
  int batch_slice = 0;  // particles per slice of a progressive batch (0 = automatic)
  double cand_voxel_ratio = 0.0;  // voxel edge / match_dist_min; 0 = chosen per map (host_map_compilers.h:build_cand_grid)
  double cand_phase = 0.5;        // grid origin shifted by this fraction of a voxel (see build_cand_grid)
  int cand_aniso = 2;             // voxel edges follow the dist_weight axis by axis (host_map_compilers.h:cand_axis_stretch): 0 never,
                                  // 1 always, 2 when cubes exceed the budget
  double cand_aniso_max = 8.0;    // ... up to this factor over the base edge
  double index_budget_opt = -1.0;   // key index_budget_bytes, as asked for: upper bound of the candidate records; -1 = a quarter of the
                                    // device's memory, 0 = none
  int cand_record_parts = 0;      // inline candidates per voxel record: 4 (64 bytes), 8 (128 bytes), 0 = chosen per map
  int cand_packed = 1;            // packed w words in the voxel records when the map allows it (map_compiler.h)
  int cand_bound = 1;             // ... with the skip bound of the overflow candidates (the bounded form) when the map allows it
  int lik_defer = 1;              // overflow rounds of the tiled kernel deferred and run densely: 0 never, 1 always
                                  // (packed 64-byte records), 2 = when more than LIK_DEFER_MIN_FRAC of the voxels overflow
  int dda_overlay = 1;      // the map update as an overlay of the DDA grid (DdaGrid::ov_*) instead of a rebuild
  int grid_build_host = 0;  // 1 = build the cell grid / the DDA grid on the host instead of from the map as a device cloud
  int beam_prepare = 1;     // per-(particle, origin) ray constants (beam_origin_kernel) for launches of at least BEAM_PREPARE_MIN_RAYS rays
  int chain_ppl = 0;          // strict_order = 3: tiles per work-group (0 = by size, 1, 4: likelihood_chain_multi.h)
  int scan_order_device = 4096;  // scans of at least this many points (both models together) are ordered on the device; 0 = never
  unsigned timing_mask = 0xffffffffu;  // bit k = time kernel group k (MCL3DL_KERNEL_*); each timed group costs two event records
};

// ---- the table -----------------------------------------------------------------------------------------------------------
// what setting a key makes the engine rebuild: the candidate index, the three grids (cell grid + base grid + DDA grid), the DDA grid
enum : unsigned
{
  EFFECT_CAND = 1u,
  EFFECT_GRIDS = 2u,
  EFFECT_DDA = 4u
};

struct OptionField  // a pointer to the member, one of the four types the options have
{
  enum Type
  {
    Int,
    Double,
    Bool,
    Unsigned
  } type;
  union
  {
    int Options::*i;
    double Options::*d;
    bool Options::*b;
    unsigned Options::*u;
  };
  constexpr OptionField(int Options::*p) : type(Int), i(p) {}
  constexpr OptionField(double Options::*p) : type(Double), d(p) {}
  constexpr OptionField(bool Options::*p) : type(Bool), b(p) {}
  constexpr OptionField(unsigned Options::*p) : type(Unsigned), u(p) {}
};

// which doubles a key takes: a flag takes any (stored as value != 0); the others one of list[0..n), compared exactly, or one
// inside lo <= value <= hi (open: value < hi) — written so that NaN is inside nothing
struct OptionRule
{
  bool flag, open;
  double lo, hi;
  double list[5];
  int n;
};
constexpr double OPTION_INF = std::numeric_limits<double>::infinity();
constexpr OptionRule flag()
{
  return { true, false, 0, 0, {}, 0 };
}
template <typename... V>
constexpr OptionRule one_of(V... v)
{
  return { false, false, 1, 0, { static_cast<double>(v)... }, static_cast<int>(sizeof...(v)) };  // lo > hi: no range
}
constexpr OptionRule range(double lo, double hi)
{
  return { false, false, lo, hi, {}, 0 };
}
constexpr OptionRule range_open(double lo, double hi)
{
  return { false, true, lo, hi, {}, 0 };
}
constexpr OptionRule value_or_range(double v, double lo, double hi)
{
  return { false, false, lo, hi, { v }, 1 };
}

struct OptionRow
{
  const char* name;
  OptionField field;
  OptionRule rule;
  const char* must;         // the error text behind "<name> must " ("" where the rule refuses nothing)
  unsigned on_change = 0;   // EFFECT_* when the stored value changes
  unsigned always = 0;      // EFFECT_* on every accepted call
  bool test_hook = false;   // needs MCL3DL_HIP_TEST_HOOKS=1, cannot be read back
};

// Values are converted to the field's type AFTER the rule has accepted them (static_cast: lik_tiled_min 1.5 stores 1), and
// "changed" compares what is stored before and after.
constexpr OptionRow kOptions[] = {
  { "lik_index", &Options::lik_index, one_of(0, 2), "be 0 (27-cell scan) or 2 (candidate records)", EFFECT_CAND },
  { "cand_voxel_ratio", &Options::cand_voxel_ratio, value_or_range(0, 0.125, 2), "be 0 (chosen per map) or in [0.125, 2]", EFFECT_CAND },
  { "cand_aniso", &Options::cand_aniso, one_of(0, 1, 2), "be 0 (cubes), 1 (boxes that follow the dist_weight) or 2 (boxes when cubes exceed the budget)", EFFECT_CAND },
  { "cand_aniso_max", &Options::cand_aniso_max, range(1, 64), "be in [1, 64]", EFFECT_CAND },
  { "index_budget_bytes", &Options::index_budget_opt, value_or_range(-1, 0, OPTION_INF), "be >= 0 (0 = no budget) or -1 (a quarter of the device's memory)", EFFECT_CAND },
  { "strict_order", &Options::strict_order, one_of(0, 1, 2, 3), "be 0 (never), 1 (always, weights too), 2 (large scans only) or 3 (always, in the engine's scan order)" },
  { "update_small", &Options::update_small, flag(), "" },
  { "update_stage", &Options::update_stage, flag(), "" },
  { "update_zero_copy", &Options::update_zero_copy, flag(), "" },
  { "poll_sync", &Options::poll_sync, one_of(0, 1, 2), "be 0, 1 or 2" },
  { "test_late_structures", &Options::test_late_structures, flag(), "", 0, 0, true },
  { "poll_spin_us", &Options::poll_spin_us, range(0, 1e9), "be >= 0" },
  { "chain_ppl", &Options::chain_ppl, one_of(0, 1, 4), "be 0 (by size), 1 or 4" },
  { "dda_overlay", &Options::dda_overlay, flag(), "", 0, EFFECT_DDA },
  { "cand_prune_coop", &Options::cand_prune_coop, flag(), "" },
  { "batch_slice", &Options::batch_slice, range(0, 1e9), "be a particle count (0 = automatic)" },
  { "update_small_conformant", &Options::update_small_conformant, flag(), "" },
  { "update_small_max", &Options::update_small_max, range(1, 65536), "be in [1, 65536]" },
  { "scan_presorted", &Options::scan_presorted, flag(), "" },
  { "strict_chunk", &Options::strict_chunk, value_or_range(0, 1024, 1e9), "be 0 (replay the scan in one piece) or a point count >= 1024" },
  { "strict_auto_min", &Options::strict_auto_min, range(1, 2147483647), "be a positive point count" },
  // strict_order 2: scans of at most this many points are added up in the caller's order, as floats (0 = none)
  { "strict_exact_max", &Options::strict_exact_max, range(0, 2147483647), "be a point count >= 0" },
  { "strict_auto_max_bytes", &Options::strict_auto_max_bytes, range(0, OPTION_INF), "be >= 0" },
  { "timing_mask", &Options::timing_mask, range_open(0, 4294967296.0), "be a 32-bit mask, in [0, 2^32)" },
  { "overlap_models", &Options::overlap_models, flag(), "" },
  { "lik_small", &Options::lik_small, flag(), "" },
  { "lik_tiled", &Options::lik_tiled, flag(), "" },
  { "lik_tiled_min", &Options::lik_tiled_min, range(1, 1e9), "be >= 1" },
  { "lik_group", &Options::lik_group, one_of(0, 4, 8, 16, 32), "be 0 (chosen per launch), 4, 8, 16 or 32" },
  { "scan_order_device", &Options::scan_order_device, range(0, 2e9), "be >= 0" },
  { "pf_fused", &Options::pf_fused, flag(), "" },
  { "lik_coop", &Options::lik_coop, flag(), "" },
  // (the record size of a crowded map follows lik_defer: host_map_compilers.h:build_cand_grid)
  { "lik_defer", &Options::lik_defer, one_of(0, 1, 2), "be 0 (never), 1 (whenever the records allow it) or 2 (crowded maps only)", EFFECT_CAND },
  { "cand_bound", &Options::cand_bound, flag(), "", EFFECT_CAND },
  { "beam_prepare", &Options::beam_prepare, flag(), "" },
  { "cand_packed", &Options::cand_packed, flag(), "", EFFECT_CAND },
  { "grid_build_host", &Options::grid_build_host, flag(), "", EFFECT_GRIDS },
  { "cand_record_parts", &Options::cand_record_parts, one_of(0, 4, 8), "be 0 (chosen per map), 4 (64-byte records) or 8 (128-byte records)", EFFECT_CAND },
  { "cand_phase", &Options::cand_phase, range_open(0, 1), "be in [0, 1)", EFFECT_CAND },
};

// ---- the interpreter -----------------------------------------------------------------------------------------------------
inline const OptionRow* option_find(const char* name)
{
  for (const OptionRow& r : kOptions)
    if (strcmp(r.name, name) == 0)
      return &r;
  return nullptr;
}

// the one gate of everything that exists for the tests alone
inline bool test_hooks_enabled()
{
  const char* hooks = getenv("MCL3DL_HIP_TEST_HOOKS");
  return hooks && strcmp(hooks, "1") == 0;
}

inline bool option_accepts(const OptionRule& r, double v)
{
  for (int k = 0; k < r.n; ++k)
    if (v == r.list[k])
      return true;
  return r.flag || (v >= r.lo && (r.open ? v < r.hi : v <= r.hi));
}

inline double option_load(const Options& opt, const OptionField& f)
{
  return f.type == OptionField::Int      ? opt.*f.i
         : f.type == OptionField::Double ? opt.*f.d
         : f.type == OptionField::Bool   ? opt.*f.b
                                         : opt.*f.u;
}

struct OptionSet
{
  int code;          // 0, or -3 with msg
  unsigned effects;  // EFFECT_*
  char msg[512];
};

inline OptionSet option_set(Options& opt, const char* name, double value)
{
  OptionSet out{ -3, 0u, "" };
  const OptionRow* row = option_find(name);
  if (!row)
    snprintf(out.msg, sizeof(out.msg), "unknown option '%s'", name);
  else if (row->test_hook && !test_hooks_enabled())
    snprintf(out.msg, sizeof(out.msg), "%s is a test hook: set MCL3DL_HIP_TEST_HOOKS=1 in the environment to enable it", name);
  else if (!option_accepts(row->rule, value))
    snprintf(out.msg, sizeof(out.msg), "%s must %s", name, row->must);
  else
  {
    const OptionField& f = row->field;
    const double before = option_load(opt, f), v = row->rule.flag ? static_cast<double>(value != 0.0) : value;
    if (f.type == OptionField::Int)
      opt.*f.i = static_cast<int>(v);
    else if (f.type == OptionField::Double)
      opt.*f.d = v;
    else if (f.type == OptionField::Bool)
      opt.*f.b = v != 0.0;
    else
      opt.*f.u = static_cast<unsigned>(v);
    out.code = 0;
    out.effects = row->always | (option_load(opt, f) != before ? row->on_change : 0u);
  }
  return out;
}

// false = no such key among the readable ones
inline bool option_get(const Options& opt, const char* name, double* value)
{
  const OptionRow* row = option_find(name);
  if (!row || row->test_hook)
    return false;
  *value = option_load(opt, row->field);
  return true;
}
