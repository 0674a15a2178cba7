// api_support.inl — included inside the extern "C" block of mcl3dl_hip.hip: kernel timing, footprint, options.
// ---- measurement support ---------------------------------------------------------------------------------------
int mcl3dl_hip_set_kernel_timing(mcl3dl_hip_ctx* ctx, int enable)
{
  if (!ctx)
    return -1;
  TRY(timing_collect(ctx));
  ctx->timing = enable != 0;
  return 0;
}

int mcl3dl_hip_get_kernel_time(mcl3dl_hip_ctx* ctx, int kernel_id, double* total_ms, uint64_t* launches)
{
  if (!ctx)
    return -1;
  if (kernel_id < 0 || kernel_id >= MCL3DL_KERNEL_COUNT)
    return ctx->fail(-3, "bad kernel id");
  TRY(timing_collect(ctx));
  if (total_ms)
    *total_ms = ctx->kernel_ms[kernel_id];
  if (launches)
    *launches = ctx->kernel_launches[kernel_id];
  return 0;
}

int mcl3dl_hip_reset_kernel_time(mcl3dl_hip_ctx* ctx)
{
  if (!ctx)
    return -1;
  TRY(timing_collect(ctx));
  for (int k = 0; k < MCL3DL_KERNEL_COUNT; ++k)
  {
    ctx->kernel_ms[k] = 0;
    ctx->kernel_launches[k] = 0;
  }
  return 0;
}

int mcl3dl_hip_memory_footprint(mcl3dl_hip_ctx* ctx, uint64_t* bytes8)
{
  if (!ctx || !bytes8)
    return -1;
  for (int i = 0; i < 8; ++i)
    bytes8[i] = ctx->footprint[i];
  return 0;
}

// Switches between two forms of one kernel that compute the same bits: set and read through the same two calls as the options,
// but no rows of host_options.h's table — nothing a caller tunes, they exist for A/B runs and for the tests that hold one form
// against the other.
namespace
{
struct Switch
{
  const char* name;
  int Options::*field;
  OptionRule rule;
  const char* must;
};
const Switch kSwitches[] = {
    { "lik_tiled_fast", &Options::lik_tiled_fast, one_of(-1, 0), "be -1 (where the map and the parameters allow it) or 0 (never)" },
};
}  // namespace

// The keys, their rules and their effects are the table of host_options.h; here the effects meet the engine's state.
int mcl3dl_hip_set_option(mcl3dl_hip_ctx* ctx, const char* name, double value)
{
  if (!ctx || !name)
    return -1;
  for (const Switch& s : kSwitches)
    if (strcmp(s.name, name) == 0)
    {
      if (!option_accepts(s.rule, value))
        return ctx->fail(-3, "%s must %s", s.name, s.must);
      ctx->opt.*s.field = static_cast<int>(value);
      return 0;
    }
  const OptionSet set = option_set(ctx->opt, name, value);
  if (set.effects & EFFECT_CAND)
    ctx->cand_dirty = true;
  if (set.effects & EFFECT_GRIDS)
    ctx->lik_dirty = ctx->lik_base_dirty = true;
  if (set.effects & (EFFECT_GRIDS | EFFECT_DDA))
    ctx->dda_dirty = true;
  return set.code == 0 ? 0 : ctx->fail(set.code, "%s", set.msg);
}

// Every option that can be set can be read back (the same table); next to them the read-only diagnostics, which need the
// context: what the index in place was built with, the counters of the map path, build times.
namespace
{
struct Diagnostic
{
  const char* name;
  double (*get)(const mcl3dl_hip_ctx*);
};
const Diagnostic kDiagnostics[] = {
    { "index_budget_in_use", [](const mcl3dl_hip_ctx* c) -> double { return c->index_budget_bytes; } },
    { "cand_aniso_active", [](const mcl3dl_hip_ctx* c) -> double { return c->cand_aniso_active ? 1.0 : 0.0; } },
    { "cand_edge_ratio_x", [](const mcl3dl_hip_ctx* c) -> double { return c->cand_edge_ratio[0]; } },
    { "cand_edge_ratio_y", [](const mcl3dl_hip_ctx* c) -> double { return c->cand_edge_ratio[1]; } },
    { "cand_edge_ratio_z", [](const mcl3dl_hip_ctx* c) -> double { return c->cand_edge_ratio[2]; } },
    // geometry of the candidate grid in place (zeros before the first build): float origin, fp64 edges, voxel counts, slack of V+
    { "cand_origin_x", [](const mcl3dl_hip_ctx* c) -> double { return c->cand_cp.ox; } },
    { "cand_origin_y", [](const mcl3dl_hip_ctx* c) -> double { return c->cand_cp.oy; } },
    { "cand_origin_z", [](const mcl3dl_hip_ctx* c) -> double { return c->cand_cp.oz; } },
    { "cand_edge_x", [](const mcl3dl_hip_ctx* c) -> double { return c->cand_cp.ex; } },
    { "cand_edge_y", [](const mcl3dl_hip_ctx* c) -> double { return c->cand_cp.ey; } },
    { "cand_edge_z", [](const mcl3dl_hip_ctx* c) -> double { return c->cand_cp.ez; } },
    { "cand_voxels_x", [](const mcl3dl_hip_ctx* c) -> double { return c->cand_cp.nvx; } },
    { "cand_voxels_y", [](const mcl3dl_hip_ctx* c) -> double { return c->cand_cp.nvy; } },
    { "cand_voxels_z", [](const mcl3dl_hip_ctx* c) -> double { return c->cand_cp.nvz; } },
    { "cand_grow", [](const mcl3dl_hip_ctx* c) -> double { return c->cand_cp.grow; } },
    { "index_record_bytes", [](const mcl3dl_hip_ctx* c) -> double { return static_cast<double>(c->footprint[6]); } },
    { "index_note", [](const mcl3dl_hip_ctx* c) -> double { return c->index_note.empty() ? 0.0 : 1.0; } },
    { "cand_record_parts_in_use", [](const mcl3dl_hip_ctx* c) -> double { return c->cand_parts; } },
    { "cand_voxels_over8", [](const mcl3dl_hip_ctx* c) -> double { return c->cand_over8; } },
    { "cand_ovf_compactions", [](const mcl3dl_hip_ctx* c) -> double { return static_cast<double>(c->cand_ovf_compactions); } },
    { "cand_ovf_leaked", [](const mcl3dl_hip_ctx* c) -> double { return c->cand_ovf_leaked; } },
    { "lik_exact", [](const mcl3dl_hip_ctx* c) -> double { return c->lik_exact ? 1.0 : 0.0; } },
    { "scan_chunk_in_use", [](const mcl3dl_hip_ctx* c) -> double { return static_cast<double>(c->scan_chunk); } },
    { "lik_grid_merges", [](const mcl3dl_hip_ctx* c) -> double { return static_cast<double>(c->lik_grid_merges); } },
    { "lik_grid_rebuilds", [](const mcl3dl_hip_ctx* c) -> double { return static_cast<double>(c->lik_grid_rebuilds); } },
    { "strict_auto_skipped", [](const mcl3dl_hip_ctx* c) -> double { return static_cast<double>(c->strict_auto_skipped); } },
    { "dda_overlay_updates", [](const mcl3dl_hip_ctx* c) -> double { return static_cast<double>(c->dda_overlay_updates); } },
    { "dda_overlay_points", [](const mcl3dl_hip_ctx* c) -> double { return c->dda_dirty ? 0.0 : static_cast<double>(c->dg.ov_n); } },
    { "batch_slices_run", [](const mcl3dl_hip_ctx* c) -> double { return static_cast<double>(c->batch_slices_run); } },
    { "lik_defer_active", [](const mcl3dl_hip_ctx* c) -> double { return lik_defer_active(c) ? 1.0 : 0.0; } },
    { "lik_tiled_fast_active", [](const mcl3dl_hip_ctx* c) -> double { return lik_tiled_fast_active(c, lik_params(c)) ? 1.0 : 0.0; } },
    { "cand_packed_active", [](const mcl3dl_hip_ctx* c) -> double { return c->rg.packed; } },
    { "cand_bound_active", [](const mcl3dl_hip_ctx* c) -> double { return c->rg.bound_step > 0.0f ? 1.0 : 0.0; } },
    { "lik_grid_build_ms", [](const mcl3dl_hip_ctx* c) -> double { return c->grid_build_ms[0]; } },
    { "dda_grid_build_ms", [](const mcl3dl_hip_ctx* c) -> double { return c->grid_build_ms[1]; } },
    { "lik_grid_build_wall_ms", [](const mcl3dl_hip_ctx* c) -> double { return c->grid_build_wall_ms[0]; } },
    { "dda_grid_build_wall_ms", [](const mcl3dl_hip_ctx* c) -> double { return c->grid_build_wall_ms[1]; } },
};
}  // namespace

int mcl3dl_hip_get_option(mcl3dl_hip_ctx* ctx, const char* name, double* value)
{
  if (!ctx || !name || !value)
    return -1;
  if (option_get(ctx->opt, name, value))
    return 0;
  for (const Switch& s : kSwitches)
    if (strcmp(s.name, name) == 0)
    {
      *value = ctx->opt.*s.field;
      return 0;
    }
  for (const Diagnostic& d : kDiagnostics)
    if (strcmp(d.name, name) == 0)
    {
      *value = d.get(ctx);
      return 0;
    }
  return ctx->fail(-3, "unknown option '%s'", name);
}

// ---- page-locked host memory for the caller's arrays ---------------------------------------------------------------------
int mcl3dl_hip_host_alloc(mcl3dl_hip_ctx* ctx, size_t bytes, void** out)
{
  if (!ctx || !out)
    return -1;
  *out = nullptr;
  if (bytes == 0)
    return ctx->fail(-3, "mcl3dl_hip_host_alloc of 0 bytes");
  HIP_TRY(hipSetDevice(ctx->device));
  void* p = pinned_alloc(ctx, bytes);
  if (!p)
    return ctx->fail(-2, "hipHostMalloc of %zu bytes failed", bytes);
  ctx->pinned.push_back({ static_cast<char*>(p), bytes });
  *out = p;
  return 0;
}

int mcl3dl_hip_host_free(mcl3dl_hip_ctx* ctx, void* p)
{
  if (!ctx)
    return -1;
  if (!p)
    return 0;
  for (size_t k = 0; k < ctx->pinned.size(); ++k)
    if (ctx->pinned[k].p == p)
    {
      HIP_TRY(hipSetDevice(ctx->device));
      TRY(sync_stream(ctx));  // nothing in flight reads or writes it
      HIP_TRY(hipHostFree(p));
      ctx->pinned.erase(ctx->pinned.begin() + static_cast<long>(k));
      return 0;
    }
  return ctx->fail(-3, "mcl3dl_hip_host_free: not a block of mcl3dl_hip_host_alloc");
}

int mcl3dl_hip_index_stats(mcl3dl_hip_ctx* ctx, double* stats8)
{
  if (!ctx || !stats8)
    return -1;
  for (int i = 0; i < 8; ++i)
    stats8[i] = ctx->cand_stats[i];
  return 0;
}
