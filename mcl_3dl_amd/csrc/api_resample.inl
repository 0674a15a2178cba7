// api_resample.inl — included inside the extern "C" block of mcl3dl_hip.hip.
// ---- "next" row: resample / resizeParticle ---------------------------------------------------------------------------
namespace
{
// std::sort(particles_dup_) over ctx->rs_keys in particle order (pf.h:200 / 408): the keys sorted, rs_order = who sits where
void resample_sort_ties(mcl3dl_hip_ctx* ctx, size_t n)
{
  std::vector<std::pair<float, uint32_t>> dup(n);
  for (size_t i = 0; i < n; ++i)
    dup[i] = { ctx->rs_keys[i], static_cast<uint32_t>(i) };
  std::sort(dup.begin(), dup.end(),
            [](const std::pair<float, uint32_t>& a, const std::pair<float, uint32_t>& b) { return a.first < b.first; });
  ctx->rs_order.resize(n);
  for (size_t i = 0; i < n; ++i)
  {
    ctx->rs_keys[i] = dup[i].first;
    ctx->rs_order[i] = dup[i].second;
  }
}

// The plan behind the keys in ctx->rs_d_keys, enqueued: n_out lower_bound searches (pscan = pstep * i + initial_p computed in
// the kernel for mode 0, pf.h:209; d_pscan for mode 1); pscan never decreases, so the search the reference starts at the
// previous `it` lands where the global one does and the it / it_prev walk of pf.h:204-223 / 414-434 becomes a neighbour
// comparison + an exclusive scan. d_rec: pstep / initial_p come from the device record (resample_prefix_kernels.h) instead of
// the arguments. The duplicate count is left in rs_d_flag[n_out].
int resample_plan_enqueue(mcl3dl_hip_ctx* ctx, int mode, const float* d_pscan, const ResampleRecord* d_rec, float pstep,
                          float initial_p, bool want_dup8)
{
  const size_t n = ctx->rs_n, n_out = ctx->rs_n_out;
  const int ni = static_cast<int>(n), no = static_cast<int>(n_out);
  TRY(ensure(ctx, ctx->rs_d_it, sizeof(uint32_t) * (n_out + 1)));  // [n_out] = the last search result below n
  TRY(ensure(ctx, ctx->rs_d_flag, sizeof(uint32_t) * (n_out + 1)));
  TRY(ensure(ctx, ctx->rs_d_ws, sizeof(uint32_t) * (n_out / 1023 + 8)));
  TRY(ensure(ctx, ctx->rs_d_source, sizeof(uint32_t) * n_out));
  TRY(ensure(ctx, ctx->rs_d_slot, sizeof(uint32_t) * n_out));
  uint32_t* d_it = ctx->rs_d_it.as<uint32_t>();
  uint32_t* d_flag = ctx->rs_d_flag.as<uint32_t>();
  HIP_TRY(hipMemsetAsync(d_it + n_out, 0, sizeof(uint32_t), ctx->stream));
  if (d_rec)
    hipLaunchKernelGGL(resample_lower_bound_record_kernel, dim3((no + 255) / 256), dim3(256), 0, ctx->stream,
                       ctx->rs_d_keys.as<float>(), ni, d_pscan, d_rec, no, d_it, d_it + n_out);
  else
    hipLaunchKernelGGL(resample_lower_bound_kernel, dim3((no + 255) / 256), dim3(256), 0, ctx->stream,
                       ctx->rs_d_keys.as<float>(), ni, d_pscan, pstep, initial_p, no, d_it, d_it + n_out);
  hipLaunchKernelGGL(resample_walk_kernel, dim3((no + 255) / 256), dim3(256), 0, ctx->stream, d_it, ni,
                     ctx->rs_sorted ? ctx->rs_d_order.as<uint32_t>() : static_cast<const uint32_t*>(nullptr), mode, no,
                     ctx->rs_d_source.as<uint32_t>(), d_flag);
  HIP_TRY(hipMemcpyAsync(ctx->rs_d_slot.p, d_flag, sizeof(uint32_t) * n_out, hipMemcpyDeviceToDevice, ctx->stream));
  HIP_TRY(hipMemsetAsync(d_flag + n_out, 0, sizeof(uint32_t), ctx->stream));
  TRY(device_exclusive_scan_ws(ctx, d_flag, static_cast<long long>(n_out) + 1, ctx->rs_d_ws.as<uint32_t>()));
  if (want_dup8)
  {
    TRY(ensure(ctx, ctx->rs_d_dup8, n_out));
    hipLaunchKernelGGL(resample_slot_kernel, dim3((no + 255) / 256), dim3(256), 0, ctx->stream, d_flag, no,
                       ctx->rs_d_slot.as<uint32_t>(), ctx->rs_d_dup8.as<uint8_t>());
  }
  else
    hipLaunchKernelGGL(resample_slot_kernel, dim3((no + 255) / 256), dim3(256), 0, ctx->stream, d_flag, no,
                       ctx->rs_d_slot.as<uint32_t>(), static_cast<uint8_t*>(nullptr));
  HIP_TRY(hipGetLastError());
  return 0;
}
}  // namespace

int mcl3dl_hip_resample_begin(mcl3dl_hip_ctx* ctx, const float* weight, size_t n, size_t n_out, float* out_pstep)
{
  if (!ctx)
    return -1;
  if (!weight || n == 0 || n_out == 0 || n > 0x7fffffffu || n_out > 0x7fffffffu)
    return ctx->fail(-3, "bad arguments to resample_begin");
  // accum += p.probability_ ; p.accum_probability_ = accum   (pf.h:193-197 / 401-405): a float recurrence in particle
  // order, so it runs on the host (one add per particle)
  ctx->rs_keys.resize(n);
  float accum = 0;
  bool ties = false;
  for (size_t i = 0; i < n; ++i)
  {
    const float prev = accum;
    accum += weight[i];
    ties = ties || (i > 0 && !(prev < accum));
    ctx->rs_keys[i] = accum;
  }
  // std::sort(particles_dup_) (pf.h:200 / 408). Ascending and tie-free input is left as it is by any sort; with ties
  // (weight-0 particles) libstdc++'s introsort decides who leads each tie group, so the very same std::sort runs here
  // (the comparison looks at the accumulated probability only, like Particle::operator<, pf.h:104-107).
  ctx->rs_sorted = ties;
  if (ties)
    resample_sort_ties(ctx, n);
  ctx->rs_n = n;
  ctx->rs_n_out = n_out;
  ctx->rs_pstep = accum / n_out;  // pf.h:202 / 410 (float / size_t)
  ctx->rs_planned = false;
  if (out_pstep)
    *out_pstep = ctx->rs_pstep;
  HIP_TRY(hipSetDevice(ctx->device));
  TRY(ensure(ctx, ctx->rs_d_keys, sizeof(float) * n));
  TRY(h2d(ctx, ctx->rs_d_keys.p, ctx->rs_keys.data(), sizeof(float) * n));
  if (ties)
  {
    TRY(ensure(ctx, ctx->rs_d_order, sizeof(uint32_t) * n));
    TRY(h2d(ctx, ctx->rs_d_order.p, ctx->rs_order.data(), sizeof(uint32_t) * n));
  }
  TRY(sync_stream(ctx));
  return 0;
}

int mcl3dl_hip_resample_plan(mcl3dl_hip_ctx* ctx, int mode, float initial_p, uint32_t* out_source,
                             uint8_t* out_duplicate, size_t* out_n_duplicates)
{
  if (!ctx)
    return -1;
  if (ctx->rs_n == 0)
    return ctx->fail(-5, "resample_plan before resample_begin");
  if (mode != 0 && mode != 1)
    return ctx->fail(-3, "mode must be 0 (resample) or 1 (resizeParticle)");
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t n_out = ctx->rs_n_out;
  const float* d_pscan = nullptr;
  if (mode == 1)
  {
    // pscan += pstep (pf.h:421): another float recurrence, host side
    std::vector<float> pscan(n_out);
    float acc = 0;
    for (size_t i = 0; i < n_out; ++i)
      pscan[i] = (acc += ctx->rs_pstep);
    TRY(ensure(ctx, ctx->rs_d_pscan, sizeof(float) * n_out));
    TRY(h2d(ctx, ctx->rs_d_pscan.p, pscan.data(), sizeof(float) * n_out));
    TRY(sync_stream(ctx));  // pscan dies at the end of this block
    d_pscan = ctx->rs_d_pscan.as<float>();
  }
  TRY(resample_plan_enqueue(ctx, mode, d_pscan, nullptr, ctx->rs_pstep, initial_p, out_duplicate != nullptr));
  uint32_t n_dup = 0;
  TRY(d2h(ctx, &n_dup, ctx->rs_d_flag.as<uint32_t>() + n_out, sizeof(uint32_t)));
  if (out_source)
    TRY(d2h(ctx, out_source, ctx->rs_d_source.p, sizeof(uint32_t) * n_out));
  if (out_duplicate)
    TRY(d2h(ctx, out_duplicate, ctx->rs_d_dup8.p, n_out));
  TRY(sync_stream(ctx));
  ctx->rs_n_dup = n_dup;
  ctx->rs_planned = true;
  if (out_n_duplicates)
    *out_n_duplicates = n_dup;
  return 0;
}

int mcl3dl_hip_resample_begin_device(mcl3dl_hip_ctx* ctx, const float* d_weight, size_t n, size_t n_out, float* out_pstep)
{
  if (!ctx)
    return -1;
  if (!d_weight || n == 0 || n > 0x7fffffffu)
    return ctx->fail(-3, "bad arguments to resample_begin_device");
  HIP_TRY(hipSetDevice(ctx->device));
  if (n_out == 0 || n_out > 0x7fffffffu)
    return ctx->fail(-3, "bad arguments to resample_begin_device");
  // the prefix sums are a float recurrence in particle order (pf.h:193-197): 4 bytes per particle come to the host (0.3 ms at
  // 262 144 particles; one device lane running the recurrence took 3.9 ms — that form and its option went in round 6)
  std::vector<float> w(n);
  TRY(d2h(ctx, w.data(), d_weight, sizeof(float) * n));
  TRY(sync_stream(ctx));
  return mcl3dl_hip_resample_begin(ctx, w.data(), n, n_out, out_pstep);
}

// Replaces: begin_device + the caller's uniform draw + plan, with weights that never leave the device. One wavefront runs the
// prefix recurrence with the serial loop's bits (float_prefix.h), forms pstep and — mode 0 — draws initial_p from the engine
// state handed in; the search reads both from the device record, so the plan is enqueued behind the prefix kernel without a
// host round trip, and the record comes home with the duplicate count. Route 0: that was all. Route 1: the record's tie
// flag is up — libstdc++'s introsort decides who leads each tie group (mcl3dl_hip_resample_begin), so the keys come to the
// host, the same std::sort runs, the order goes up and the plan is enqueued again over the sorted keys.
int mcl3dl_hip_resample_plan_device(mcl3dl_hip_ctx* ctx, const float* d_weight, size_t n, size_t n_out, int mode,
                                    uint32_t* engine_state, float* out_pstep, float* out_initial_p, size_t* out_n_duplicates,
                                    int* out_route)
{
  if (!ctx)
    return -1;
  if (!d_weight || n == 0 || n > 0x7fffffffu)
    return ctx->fail(-3, "bad arguments to resample_plan_device: null d_weight, or n = %zu outside [1, 2^31 - 1]", n);
  if (n_out == 0 || n_out > 0x7fffffffu)
    return ctx->fail(-3, "resample_plan_device: n_out = %zu is outside [1, 2^31 - 1]", n_out);
  if (mode != 0 && mode != 1)
    return ctx->fail(-3, "mode must be 0 (resample) or 1 (resizeParticle)");
  if (mode == 0)
    TRY(rng_check_state(ctx, engine_state));
  HIP_TRY(hipSetDevice(ctx->device));
  ctx->rs_planned = false;
  ctx->rs_n = 0;
  TRY(ensure(ctx, ctx->rs_d_keys, sizeof(float) * n));
  TRY(ensure(ctx, ctx->rs_d_rec, sizeof(ResampleRecord)));
  const ResampleRecord* d_rec = ctx->rs_d_rec.as<ResampleRecord>();
  hipLaunchKernelGGL(resample_prefix_kernel, dim3(1), dim3(64), 0, ctx->stream, d_weight, static_cast<int>(n),
                     static_cast<int>(n_out), mode, mode == 0 ? *engine_state : 0u, ctx->rs_d_keys.as<float>(),
                     ctx->rs_d_rec.as<ResampleRecord>());
  const float* d_pscan = nullptr;
  if (mode == 1)
  {
    TRY(ensure(ctx, ctx->rs_d_pscan, sizeof(float) * n_out));
    hipLaunchKernelGGL(resample_pscan_kernel, dim3(1), dim3(64), 0, ctx->stream, d_rec, static_cast<int>(n_out),
                       ctx->rs_d_pscan.as<float>());
    d_pscan = ctx->rs_d_pscan.as<float>();
  }
  HIP_TRY(hipGetLastError());
  ctx->rs_n = n;
  ctx->rs_n_out = n_out;
  ctx->rs_sorted = false;
  // (speculative: without ties this IS the plan)
  TRY(resample_plan_enqueue(ctx, mode, d_pscan, d_rec, 0.f, 0.f, false));
  ResampleRecord rec{};
  uint32_t n_dup = 0;
  TRY(d2h(ctx, &rec, d_rec, sizeof(rec)));
  TRY(d2h(ctx, &n_dup, ctx->rs_d_flag.as<uint32_t>() + n_out, sizeof(uint32_t)));
  TRY(sync_stream(ctx));
  if (rec.ties)
  {
    ctx->rs_keys.resize(n);
    TRY(d2h(ctx, ctx->rs_keys.data(), ctx->rs_d_keys.p, sizeof(float) * n));
    TRY(sync_stream(ctx));
    resample_sort_ties(ctx, n);
    ctx->rs_sorted = true;
    TRY(ensure(ctx, ctx->rs_d_order, sizeof(uint32_t) * n));
    TRY(h2d(ctx, ctx->rs_d_keys.p, ctx->rs_keys.data(), sizeof(float) * n));
    TRY(h2d(ctx, ctx->rs_d_order.p, ctx->rs_order.data(), sizeof(uint32_t) * n));
    TRY(resample_plan_enqueue(ctx, mode, d_pscan, d_rec, 0.f, 0.f, false));
    TRY(d2h(ctx, &n_dup, ctx->rs_d_flag.as<uint32_t>() + n_out, sizeof(uint32_t)));
    TRY(sync_stream(ctx));
  }
  ctx->rs_pstep = rec.pstep;
  ctx->rs_n_dup = n_dup;
  ctx->rs_planned = true;
  if (mode == 0)
    *engine_state = rec.state;
  if (out_pstep)
    *out_pstep = rec.pstep;
  if (out_initial_p)
    *out_initial_p = rec.initial_p;
  if (out_n_duplicates)
    *out_n_duplicates = n_dup;
  if (out_route)
    *out_route = rec.ties ? 1 : 0;
  return 0;
}

// The chain on its own, for introspection and tests: out_prefix[i] = fl(out_prefix[i - 1] + term i) with the serial loop's
// bits, by one wavefront. term == NULL: every term is `constant` (pscan += pstep).
int mcl3dl_hip_float_prefix(mcl3dl_hip_ctx* ctx, const float* term, float constant, size_t n, float* out_prefix)
{
  if (!ctx)
    return -1;
  if (n > 0x7fffffffu)
    return ctx->fail(-3, "float_prefix: n = %zu is more than one call takes", n);
  if (n && !out_prefix)
    return ctx->fail(-3, "null out_prefix");
  if (n == 0)
    return 0;
  HIP_TRY(hipSetDevice(ctx->device));
  TRY(ensure(ctx, ctx->rs_d_prefix, sizeof(float) * n));
  if (term)
  {
    TRY(ensure(ctx, ctx->rs_d_w, sizeof(float) * n));
    TRY(h2d(ctx, ctx->rs_d_w.p, term, sizeof(float) * n));
  }
  hipLaunchKernelGGL(float_prefix_kernel, dim3(1), dim3(64), 0, ctx->stream,
                     term ? ctx->rs_d_w.as<float>() : static_cast<const float*>(nullptr), constant, static_cast<long long>(n),
                     ctx->rs_d_prefix.as<float>());
  HIP_TRY(hipGetLastError());
  TRY(d2h(ctx, out_prefix, ctx->rs_d_prefix.p, sizeof(float) * n));
  return sync_stream(ctx);
}

namespace
{
int resample_slice_check(mcl3dl_hip_ctx* ctx, const float* d_state13_in, size_t out_begin, size_t out_count,
                         const float* d_state13_out)
{
  if (!ctx->rs_planned)
    return ctx->fail(-5, "resample_apply before resample_plan");
  if (!d_state13_in || !d_state13_out || d_state13_in == d_state13_out)
    return ctx->fail(-3, "resample_apply needs distinct input and output state arrays");
  if (out_begin > ctx->rs_n_out || out_count > ctx->rs_n_out - out_begin)
    return ctx->fail(-3, "resample_apply: slice [%zu, %zu) is outside the %zu planned slots", out_begin,
                     out_begin + out_count, ctx->rs_n_out);
  return 0;
}

// what lies behind the noise rows' arrival in ctx->rs_d_noise (copied from the host, or drawn there: api_rng.inl)
int resample_slice_launch(mcl3dl_hip_ctx* ctx, const float* d_state13_in, size_t out_begin, size_t out_count,
                          float* d_state13_out)
{
  const int no = static_cast<int>(out_count);
  hipLaunchKernelGGL(resample_apply_kernel, dim3((no + 255) / 256), dim3(256), 0, ctx->stream, d_state13_in,
                     ctx->rs_d_source.as<uint32_t>() + out_begin, ctx->rs_d_slot.as<uint32_t>() + out_begin,
                     ctx->rs_d_noise.as<float>(), no, d_state13_out);
  HIP_TRY(hipGetLastError());
  return sync_stream(ctx);  // (the noise rows may be the caller's host buffer)
}
}  // namespace

int mcl3dl_hip_resample_apply_slice_device(mcl3dl_hip_ctx* ctx, const float* d_state13_in, const float* noise13,
                                           size_t n_noise, size_t out_begin, size_t out_count, float* d_state13_out)
{
  if (!ctx)
    return -1;
  TRY(resample_slice_check(ctx, d_state13_in, out_begin, out_count, d_state13_out));
  if (n_noise < ctx->rs_n_dup || (ctx->rs_n_dup && !noise13))
    return ctx->fail(-3, "resample_apply: %zu duplicated particles need noise, %zu given", ctx->rs_n_dup, n_noise);
  if (out_count == 0)
    return 0;
  HIP_TRY(hipSetDevice(ctx->device));
  TRY(ensure(ctx, ctx->rs_d_noise, sizeof(float) * 13 * ctx->rs_n_dup));
  TRY(h2d(ctx, ctx->rs_d_noise.p, noise13, sizeof(float) * 13 * ctx->rs_n_dup));
  return resample_slice_launch(ctx, d_state13_in, out_begin, out_count, d_state13_out);
}

int mcl3dl_hip_resample_apply_device(mcl3dl_hip_ctx* ctx, const float* d_state13_in, const float* noise13,
                                     size_t n_noise, float* d_state13_out)
{
  if (!ctx)
    return -1;
  return mcl3dl_hip_resample_apply_slice_device(ctx, d_state13_in, noise13, n_noise, 0, ctx->rs_n_out, d_state13_out);
}

int mcl3dl_hip_resample_apply(mcl3dl_hip_ctx* ctx, const float* state13_in, const float* noise13, size_t n_noise,
                              float* state13_out)
{
  if (!ctx)
    return -1;
  if (!ctx->rs_planned)
    return ctx->fail(-5, "resample_apply before resample_plan");
  if (!state13_in || !state13_out)
    return ctx->fail(-3, "null state array");
  HIP_TRY(hipSetDevice(ctx->device));
  TRY(ensure(ctx, ctx->rs_d_in, sizeof(float) * 13 * ctx->rs_n));
  TRY(ensure(ctx, ctx->rs_d_out, sizeof(float) * 13 * ctx->rs_n_out));
  TRY(h2d(ctx, ctx->rs_d_in.p, state13_in, sizeof(float) * 13 * ctx->rs_n));
  TRY(mcl3dl_hip_resample_apply_device(ctx, ctx->rs_d_in.as<float>(), noise13, n_noise, ctx->rs_d_out.as<float>()));
  TRY(d2h(ctx, state13_out, ctx->rs_d_out.p, sizeof(float) * 13 * ctx->rs_n_out));
  TRY(sync_stream(ctx));
  return 0;
}

