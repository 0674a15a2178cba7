// host_pf.h — included by mcl3dl_hip.hip behind host_measure.h: pf::measure (pf_kernels.h) on the host side. Which form runs is
// decided here once, and every launch of pf_partial_kernel, lik_pf_partial_kernel, pf_reduce_kernel, pf_strict_sum_kernel,
// pf_apply_kernel and pf_fused_kernel in the library is written here once (pf_apply_kernel twice: its two forms).
namespace
{
int pf_blocks(size_t n)
{
  const size_t b = (n + PF_BLOCK - 1) / PF_BLOCK;
  return static_cast<int>(std::min<size_t>(std::max<size_t>(b, 1), 1024));
}

// ---- the decisions ------------------------------------------------------------------------------------------------------
// the particle counts of the fused work-group: up to the constant PF_FUSED_MAX_PARTICLES (1024, host_options.h; the kernel takes up
// to PF_FUSED_MAX = 4096)
static_assert(PF_FUSED_MAX_PARTICLES <= PF_FUSED_MAX, "the fused kernel's LDS row holds PF_FUSED_MAX weights");
bool pf_fused_range(size_t n_p)
{
  return n_p <= static_cast<size_t>(PF_FUSED_MAX_PARTICLES);
}

// Does pf::measure on ONE GPU add the un-normalised weights as the reference does (pf.h:255-260: float, sequentially, particle
// order; float_chain.h) instead of the fp64 tree? strict_order 1: always. The default (2): up to PF_FUSED_MAX_PARTICLES = 1024 particles —
// the reference's operating range; pf::measure is then the reference's arithmetic bit for bit given its inputs, inside the
// fused kernel / the one-launch update at no extra launch. Beyond that the recurrence needs a launch of its own
// (pf_strict_sum_kernel: +10 us at 4096 particles, a third of a 4096 x 96 update, profiles/r06d_rows_vs_replay.txt) for weights
// that agree to ~1e-7 anyway. Independent of pf_fused, so that the fused and the split form give the same bits.
bool pf_float_order(const mcl3dl_hip_ctx* ctx, size_t n_p)
{
  return ctx->opt.strict_order == 1 || (ctx->opt.strict_order == 2 && pf_fused_range(n_p));
}

// pf::measure on one GPU: the fused single-work-group kernel up to PF_FUSED_MAX_PARTICLES particles (same bits as the split form), the
// split form beyond — with the fp64 tree over the weights TWO launches since round 6 (five with lik_finalize_kernel in front
// until then): lik_pf_partial_kernel / pf_partial_kernel, then pf_apply_kernel whose every work-group runs pf_reduce_kernel's
// reduction itself. Same arithmetic in the same association as the launches apart (the multi-GPU protocol still runs them apart,
// the all-reduce between them): the same bits. Measured on one box, C2: 0.2344 -> 0.2303 ms per update, C3 0.3448 -> 0.3409
// (profiles/r06p_tail_ab.txt); the earlier forms of the idea that LOST are in profiles/r06o_pf_two_launch_ab.txt. With the
// reference's float recurrence over the weights, pf_strict_sum_kernel runs between the two halves of the multi-GPU protocol.
enum class PfForm
{
  Fused,
  SplitTree,
  SplitFloat
};
PfForm pf_form(const mcl3dl_hip_ctx* ctx, size_t n_p)
{
  if (ctx->opt.pf_fused && pf_fused_range(n_p))
    return PfForm::Fused;
  return pf_float_order(ctx, n_p) ? PfForm::SplitFloat : PfForm::SplitTree;
}

// lik_pf_partial_kernel holds one particle per thread of pf_partial_kernel's largest grid
bool pf_tiles_fit(size_t n_p)
{
  return n_p <= static_cast<size_t>(1024) * PF_BLOCK;
}
// is pf::measure of n_p particles on this GPU the split form with the fp64 sum of the weights? Then launch_measure may leave the
// sum over the tiled kernel's per-tile partials to lik_pf_partial_kernel (LikTail). (A rank of a device group never runs the
// fused form and keeps pf_reduce_kernel apart: it asks pf_tiles_fit alone.)
bool pf_takes_tiles(const mcl3dl_hip_ctx* ctx, size_t n_p)
{
  return pf_form(ctx, n_p) == PfForm::SplitTree && pf_tiles_fit(n_p);
}

// ---- one pf::measure call as its launchers see it -------------------------------------------------------------------------
struct PfCall
{
  mcl3dl_hip_ctx* ctx;
  float* d_w;  // the prior weights; the second half writes the normalised ones over them
  float* d_lik;  // (written only where launch_measure left the tiled kernel's sums: tail->pending)
  float* d_beam;  // or null
  const float* d_extra;  // or null
  float* d_ratio;  // or null
  size_t n_p;
  float* d_stats4;
  const LikTail* tail = nullptr;  // what launch_measure left to the first kernel
  const ImuGravity* model = nullptr;  // the likelihood formed inside the first kernel (d_lik may then be null)
  const PfEmit* emit = nullptr;  // page-locked arrays the last kernel writes the results to as well
  bool timed = true;  // an EventPair of category MCL3DL_KERNEL_PF around the launches

  int np() const
  {
    return static_cast<int>(n_p);
  }
  int nb() const
  {
    return pf_blocks(n_p);
  }
  bool tiles_pending() const
  {
    return tail && tail->pending;
  }
  bool beam_pending() const
  {
    return tail && tail->beam_pending;
  }
  // the form on one GPU (launch_measure leaves its tiles to the split form with the fp64 tree only: pf_takes_tiles)
  PfForm form() const
  {
    return tiles_pending() ? PfForm::SplitTree : pf_form(ctx, n_p);
  }
  // Who performs the beam model's last step (penalty counts -> scores) on one GPU? The first pf kernel through BeamCounts —
  // or, in front of the float-order split form, beam_finalize_kernel in a launch of its own after all. (A rank's first half
  // always takes the counts.)
  bool counts_in_kernel() const
  {
    return beam_pending() && form() != PfForm::SplitFloat;
  }
  // doubles of block_partials the first kernel fills (behind the tiled kernel: whole blocks of four wavefront partials)
  size_t partials_doubles() const
  {
    return static_cast<size_t>(tiles_pending() ? 16 : 4) * nb();
  }
};

// ---- the launches ---------------------------------------------------------------------------------------------------------
int pf_reserve(const PfCall& c, bool partials)
{
  TRY(ensure(c.ctx, c.ctx->wnew, sizeof(float) * c.n_p));
  if (partials)
    TRY(ensure(c.ctx, c.ctx->block_partials, sizeof(double) * c.partials_doubles()));
  return 0;
}
int pf_timing_begin(const PfCall& c, EventPair* ep)
{
  return c.timed ? timing_begin(c.ctx, MCL3DL_KERNEL_PF, ep) : 0;
}
int pf_timing_end(const PfCall& c, const EventPair& ep)
{
  mcl3dl_hip_ctx* ctx = c.ctx;
  if (c.timed)
    TRY(timing_end(ctx, ep));
  HIP_TRY(hipGetLastError());
  return 0;
}

// The first kernel: w_new = w * l and the partial sums — per block, or (launch_measure left the tiled kernel's per-tile partials
// where they are: lik_finalize_kernel's sum and pf_partial_kernel's product in one launch, pf_kernels.h) per wavefront. Returns
// the number of wavefront partials, 0 for block partials. counts: the beam score from the penalty counts on the way.
int pf_launch_partial(const PfCall& c, bool counts)
{
  mcl3dl_hip_ctx* ctx = c.ctx;
  const BeamCounts bc = counts ? BeamCounts{ ctx->penalty.as<unsigned>(), ctx->pow_table.as<float>(), ctx->beam_likelihood_min, c.d_beam }
                               : BeamCounts{ nullptr, nullptr, 0.0f, nullptr };
  int n_waves = 0;
  if (c.tiles_pending())
  {
    n_waves = static_cast<int>((c.n_p + 63) / 64);
    const LikTiles lt{ ctx->lik_partial_sum.as<double>(), ctx->lik_partial_cnt.as<unsigned>(), c.tail->n_tiles, static_cast<int>(ctx->n_s),
                       c.d_lik, c.d_ratio, c.tail->beam_fill ? c.d_beam : static_cast<float*>(nullptr), bc };
    hipLaunchKernelGGL(lik_pf_partial_kernel, dim3(n_waves), dim3(256), 0, ctx->stream, lt, c.d_w, c.d_beam, c.d_extra, c.np(),
                       ctx->wnew.as<float>(), ctx->block_partials.as<double>());
  }
  else
    hipLaunchKernelGGL(pf_partial_kernel, dim3(c.nb()), dim3(PF_BLOCK), 0, ctx->stream, c.d_w, c.d_lik, c.d_beam, c.d_extra,
                       c.d_ratio, c.np(), ctx->wnew.as<float>(), ctx->block_partials.as<double>(), bc,
                       c.model ? *c.model : ImuGravity{});
  if (counts)
    ctx->penalty_clean_n = c.n_p;  // (launched: the kernel zeroes every counter it reads)
  return n_waves;
}

// the shard's share { sum w, sum w ln w | max ratio, -min ratio per rank } of the 2 + 2 * world-double record
void pf_launch_reduce(mcl3dl_hip_ctx* ctx, const double* partials, int n_blocks, int n_waves, int rank, int world, double* d_packed)
{
  hipLaunchKernelGGL(pf_reduce_kernel, dim3(1), dim3(64), 0, ctx->stream, partials, n_blocks, rank, world, d_packed, n_waves);
}

// first half: the partial sums into the packed record; on one GPU with the float order, the reference's float recurrence over
// the weights replaces the record's sum (pf_strict_sum_kernel)
void pf_launch_first_half(const PfCall& c, bool counts, int rank, int world, double* d_packed)
{
  mcl3dl_hip_ctx* ctx = c.ctx;
  const int n_waves = pf_launch_partial(c, counts);
  pf_launch_reduce(ctx, ctx->block_partials.as<double>(), c.nb(), n_waves, rank, world, d_packed);
  if (world == 1 && pf_float_order(ctx, c.n_p))
    hipLaunchKernelGGL(pf_strict_sum_kernel, dim3(1), dim3(256), 0, ctx->stream, ctx->wnew.as<float>(), c.np(), d_packed);
}

// second half: the weights normalised by the record's sum, the four statistics; emit: the results into page-locked memory too
void pf_launch_second_half(const PfCall& c, int world, const double* d_packed)
{
  mcl3dl_hip_ctx* ctx = c.ctx;
  const auto src = [&](const float* p) { return c.emit ? p : nullptr; };  // (read for the emission only)
  hipLaunchKernelGGL(pf_apply_kernel, dim3(c.nb()), dim3(PF_BLOCK), 0, ctx->stream, c.d_w, ctx->wnew.as<float>(), c.np(), world,
                     d_packed, c.d_stats4, c.emit ? *c.emit : PfEmit{}, src(c.d_lik), src(c.d_ratio), src(c.d_beam));
}

// ---- the three sequencers -------------------------------------------------------------------------------------------------
// First half of pf::measure for rank `rank` of `world` (the packed layout of the update's one all-reduce), with the two steps
// launch_measure may have left to it (c.tail): the sum over the tiled kernel's per-tile partials and the beam model's penalty
// count -> score. Same arithmetic in the same association as the launches apart: the same bits.
int pf_first_half(const PfCall& c, int rank, int world, double* d_packed)
{
  TRY(pf_reserve(c, true));
  EventPair ep{};
  TRY(pf_timing_begin(c, &ep));
  pf_launch_first_half(c, c.beam_pending(), rank, world, d_packed);
  return pf_timing_end(c, ep);
}

// ... of a shard that holds no particle: sums 0, max ratio 0, -min ratio -1
int pf_first_half_empty(mcl3dl_hip_ctx* ctx, int rank, int world, double* d_packed)
{
  pf_launch_reduce(ctx, nullptr, 0, 0, rank, world, d_packed);
  HIP_TRY(hipGetLastError());
  return 0;
}

int pf_second_half(const PfCall& c, int world, const double* d_packed)
{
  EventPair ep{};
  TRY(pf_timing_begin(c, &ep));
  pf_launch_second_half(c, world, d_packed);
  return pf_timing_end(c, ep);
}

// pf::measure on one GPU (ctx->partial4 ensured by the caller)
int pf_one_gpu(const PfCall& c)
{
  mcl3dl_hip_ctx* ctx = c.ctx;
  const PfForm form = c.form();
  const bool counts = c.counts_in_kernel();
  if (c.beam_pending() && !counts)
    hipLaunchKernelGGL(beam_finalize_kernel, dim3((static_cast<unsigned>(c.n_p) + 255) / 256), dim3(256), 0, ctx->stream,
                       ctx->penalty.as<unsigned>(), ctx->pow_table.as<float>(), ctx->beam_likelihood_min, c.d_beam, c.np());
  TRY(pf_reserve(c, form != PfForm::Fused));
  EventPair ep{};
  TRY(pf_timing_begin(c, &ep));
  if (form == PfForm::Fused)
  {
    const BeamCounts bc = counts ? BeamCounts{ ctx->penalty.as<unsigned>(), ctx->pow_table.as<float>(), ctx->beam_likelihood_min, c.d_beam }
                                 : BeamCounts{ nullptr, nullptr, 0.0f, nullptr };
    hipLaunchKernelGGL(pf_fused_kernel, dim3(1), dim3(1024), 0, ctx->stream, c.d_w, c.d_lik, c.d_beam, c.d_extra, c.d_ratio, c.np(),
                       ctx->wnew.as<float>(), ctx->partial4.as<double>(), c.d_stats4, c.emit ? *c.emit : PfEmit{},
                       pf_float_order(ctx, c.n_p) ? 1 : 0, bc, c.model ? *c.model : ImuGravity{});
    if (counts)
      ctx->penalty_clean_n = c.n_p;  // (launched: the kernel zeroes every counter it reads)
  }
  else if (form == PfForm::SplitTree)
  {
    const int n_waves = pf_launch_partial(c, counts);
    hipLaunchKernelGGL(pf_apply_kernel, dim3(c.nb()), dim3(PF_BLOCK), 0, ctx->stream, c.d_w, ctx->wnew.as<float>(), c.np(), 1,
                       static_cast<const double*>(nullptr), c.d_stats4, c.emit ? *c.emit : PfEmit{}, c.d_lik, c.d_ratio, c.d_beam,
                       ctx->block_partials.as<double>(), c.nb(), n_waves, ctx->partial4.as<double>());
  }
  else
  {
    pf_launch_first_half(c, false, 0, 1, ctx->partial4.as<double>());
    pf_launch_second_half(c, 1, ctx->partial4.as<double>());
  }
  return pf_timing_end(c, ep);
}
}  // namespace
