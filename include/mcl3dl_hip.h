/* mcl3dl_hip.h — C ABI of the MI355X-native LiDAR measurement-update engine for mcl_3dl.
 *
 * This is the drop-in boundary: plain C, plain pointers and sizes, no C++/torch types.
 * Each entry point names the reference interface it replaces (paths relative to the at-wat/mcl_3dl
 * v0.7.0 tree).  The C++ adapter classes in mcl_3dl_amd/cpp/include/ (same class names as the
 * reference's plugins) and the ctypes binding mcl_3dl_amd/capi.py both sit on top of exactly these symbols.
 *
 * Conventions
 *   - every function returning int: 0 = OK, negative = error; mcl3dl_hip_last_error(ctx) has the text.
 *   - the caller owns every host buffer; the context owns all device memory. One context = one GPU;
 *     a context is not thread-safe (the reference caller is single-threaded: src/mcl_3dl.cpp:1466).
 *   - arrays are contiguous, little-endian, float32 unless stated.  pose = 7 floats per particle:
 *     px,py,pz (State6DOF::pos_), qx,qy,qz,qw (State6DOF::rot_, NOT required to be normalised).
 *   - "host" entry points take host pointers and are synchronous; "device" entry points take device
 *     pointers, enqueue on the context's stream and return without synchronising.
 *   - There is no CPU fallback: without a usable gfx950 device mcl3dl_hip_create fails.
 */
#ifndef MCL3DL_HIP_H
#define MCL3DL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCL3DL_HIP_ABI_VERSION 3

typedef struct mcl3dl_hip_ctx mcl3dl_hip_ctx;

/* BeamStatus, include/mcl_3dl/lidar_measurement_models/lidar_measurement_model_beam.h:64-70 (same order). */
enum
{
  MCL3DL_BEAM_SHORT = 0,
  MCL3DL_BEAM_HIT = 1,
  MCL3DL_BEAM_LONG = 2,
  MCL3DL_BEAM_TOTAL_REFLECTION = 3
};

/* kernel ids for mcl3dl_hip_get_kernel_time */
enum
{
  MCL3DL_KERNEL_LIKELIHOOD = 0,
  MCL3DL_KERNEL_BEAM = 1,
  MCL3DL_KERNEL_PF = 2,
  MCL3DL_KERNEL_UPDATE = 3, /* the whole update as one launch (<= update_small_max particles): likelihood + beam + pf::measure */
  MCL3DL_KERNEL_STAGE = 4,  /* scan_stage_kernel of a host-buffer update: scan ordering + pose / weight take-over */
  MCL3DL_KERNEL_COUNT = 5
};

int mcl3dl_hip_abi_version(void);

/* ---- lifecycle ------------------------------------------------------------------------------------ */
/* Replaces: construction of the two LiDAR models + kd-tree in MCL3dlNode (src/mcl_3dl.cpp:1315-1329). */
/* Number of HIP devices this process sees (0 when there is none: the library has no CPU path). */
int mcl3dl_hip_device_count(void);
/* The environment variable MCL3DL_HIP_OPTIONS ("name=value,name=value", names of mcl3dl_hip_set_option) is applied to every
 * context at creation; an entry that mcl3dl_hip_set_option rejects fails the creation (-3, reason on stderr). */
int mcl3dl_hip_create(mcl3dl_hip_ctx** out, int device_id);
void mcl3dl_hip_destroy(mcl3dl_hip_ctx* ctx);
const char* mcl3dl_hip_last_error(const mcl3dl_hip_ctx* ctx);
/* Use an existing hipStream_t (e.g. the host framework's current stream); NULL = the context's own (non-blocking)
 * stream. To run on the legacy default stream pass hipStreamLegacy, not NULL. */
int mcl3dl_hip_set_stream(mcl3dl_hip_ctx* ctx, void* hip_stream);
void* mcl3dl_hip_get_stream(mcl3dl_hip_ctx* ctx);
int mcl3dl_hip_synchronize(mcl3dl_hip_ctx* ctx);

/* ---- map + parameters ------------------------------------------------------------------------------ */
/* Replaces: ChunkedKdtree::setInputCloud (include/mcl_3dl/chunked_kdtree.h:124-216, called at
 * src/mcl_3dl.cpp:1369) and RaycastUsingDDA::updatePointCloud (include/mcl_3dl/raycasts/raycast_using_dda.h:162-190).
 * dist_weight = the PointRepresentation rescale values (src/mcl_3dl.cpp:1270), NULL = none.
 * The device structures are (re)built lazily, keyed on `stamp` like raycast_using_dda.h:168. */
int mcl3dl_hip_set_map(mcl3dl_hip_ctx* ctx, const float* xyz /*n_m*3*/, const uint32_t* label /*n_m or NULL*/,
                       size_t n_m, uint64_t stamp, const float* dist_weight /*3 or NULL*/);
/* Replaces: LidarMeasurementModelLikelihoodParameters + refreshParameters
 * (include/mcl_3dl/parameters.h:64-89, src/lidar_measurement_model_likelihood.cpp:56-61). */
int mcl3dl_hip_set_likelihood_params(mcl3dl_hip_ctx* ctx, float match_dist_min, float match_dist_flat,
                                     float match_weight);
/* Replaces: LidarMeasurementModelBeamParameters + refreshParameters with use_raycast_using_dda = true
 * (include/mcl_3dl/parameters.h:91-132, src/lidar_measurement_model_beam.cpp:58-80). num_points is
 * num_points_default_ (it defines beam_likelihood_ = pow(beam_likelihood_min, 1/num_points)). */
int mcl3dl_hip_set_beam_params(mcl3dl_hip_ctx* ctx, float map_grid_x, float map_grid_y, float map_grid_z,
                               float dda_grid_size, float ray_angle_half, float hit_range, float beam_likelihood_min,
                               uint32_t num_points, float ang_total_ref, uint32_t filter_label_max,
                               int add_penalty_short_only_mode);
/* Replaces: the choice of raycaster in LidarMeasurementModelBeam::refreshParameters (src/lidar_measurement_model_beam.cpp:69-79)
 * by beam/use_raycast_using_dda (include/mcl_3dl/parameters.h:109, src/parameters.cpp:289 — false by default there).
 * mode 0 = RaycastUsingDDA (include/mcl_3dl/raycasts/raycast_using_dda.h; this library's default and its fast path),
 * mode 1 = RaycastUsingKDTree (include/mcl_3dl/raycasts/raycast_using_kdtree.h:58-109): steps of the smallest map_grid edge,
 * at each a ChunkedKdtree::radiusSearch (mcl3dl_hip_radius_search's definition, exact) and the surface's inclination from
 * a second search — the only caster that reports TOTAL_REFLECTION. Mode 1 uses map_grid_x/y/z, hit_range (the caster's
 * hit_tolerance_), beam_likelihood_min, num_points, ang_total_ref, filter_label_max and add_penalty_short_only_mode of
 * mcl3dl_hip_set_beam_params and ignores dda_grid_size and ray_angle_half. Any other mode: -3. May be changed at any time;
 * the next call that casts rays (measure_batch, measure_update, measure_device, update_device, beam_status, the group
 * forms) uses it. mcl3dl_hip_dda_trace stays on the DDA caster. */
int mcl3dl_hip_set_beam_raycast(mcl3dl_hip_ctx* ctx, int mode);
/* Replaces: reading LidarMeasurementModelBeamParameters::use_raycast_using_dda_ back (include/mcl_3dl/parameters.h:109):
 * *mode = 0 (DDA) or 1 (kd-tree). */
int mcl3dl_hip_get_beam_raycast(mcl3dl_hip_ctx* ctx, int* mode);

/* ---- host entry points (synchronous) ------------------------------------------------------------- */
/* Replaces: the N_p calls of LidarMeasurementModelLikelihood::measure
 * (src/lidar_measurement_model_likelihood.cpp:105-139) and LidarMeasurementModelBeam::measure
 * (src/lidar_measurement_model_beam.cpp:124-155) made by the measure lambda (src/mcl_3dl.cpp:409-415).
 * n_s == 0 -> out_lik = 1, out_match_ratio = 0; n_b == 0 -> out_beam = 1 (the (1,0) of an empty cloud).
 * scan_beam_origin[i] = PointXYZIL::label of beam point i = index into origins. Any out_* may be NULL. */
/* Upload the particle poses once per update; measure_batch calls with pose == NULL and the same n_p then use them. The
 * node asks each model separately (src/mcl_3dl.cpp:409-415): with this the drop-in classes send the poses once per
 * pf::measure, not once per model. Any host-buffer call that is given a pose array replaces the uploaded set. The pose array
 * may be reused as soon as the call returns (it does not wait for the stream unless the copy could not be staged). */
int mcl3dl_hip_upload_poses(mcl3dl_hip_ctx* ctx, const float* pose /*n_p*7*/, size_t n_p);
int mcl3dl_hip_measure_batch(mcl3dl_hip_ctx* ctx, const float* pose /*n_p*7 or NULL*/, size_t n_p,
                             const float* scan_lik_xyz /*n_s*3*/, size_t n_s, const float* scan_beam_xyz /*n_b*3*/,
                             const uint32_t* scan_beam_origin /*n_b*/, size_t n_b, const float* origins /*n_o*3*/,
                             size_t n_o, float* out_lik /*n_p*/, float* out_match_ratio /*n_p*/,
                             float* out_beam /*n_p*/);

/* measure_batch delivered in particle order while the GPU is still working — for a caller that consumes the results one
 * particle at a time on the host, which is what the reference's pf::measure does with the lambda of src/mcl_3dl.cpp:399-426
 * (include/mcl_3dl/pf.h:255-260: ~80 ns of host work per particle, 0.34 ms at 4096 particles — longer than the kernels).
 *   _begin  same arguments as measure_batch + slice_particles (0 = option "batch_slice", itself 0 = automatic: four slices,
 *           none below 512 particles; batches under 1024 particles are not sliced). Enqueues everything and returns; the
 *           INPUT arrays may be reused at once (they were copied or are page-locked memory the kernels read in place — the
 *           latter must stay untouched until _end), the OUTPUT arrays belong to the batch until _end.
 *   _wait   returns once out_*[particle] are valid; *n_ready (optional) = number of leading particles whose results are
 *           valid, so that a loop calls _wait once per slice, not once per particle.
 *   _end    all results delivered (also implied by any other call on the context that synchronises its stream).
 * Results are those of measure_batch bit for bit (a particle's result does not depend on which particles share its launch). */
int mcl3dl_hip_measure_batch_begin(mcl3dl_hip_ctx* ctx, const float* pose /*n_p*7 or NULL*/, size_t n_p,
                                   const float* scan_lik_xyz, size_t n_s, const float* scan_beam_xyz,
                                   const uint32_t* scan_beam_origin, size_t n_b, const float* origins, size_t n_o,
                                   float* out_lik, float* out_match_ratio, float* out_beam, size_t slice_particles);
int mcl3dl_hip_measure_batch_wait(mcl3dl_hip_ctx* ctx, size_t particle, size_t* n_ready);
int mcl3dl_hip_measure_batch_end(mcl3dl_hip_ctx* ctx);

/* Replaces: pf::ParticleFilter::measure (include/mcl_3dl/pf.h:252-279) given the per-particle factors of the
 * measure lambda (src/mcl_3dl.cpp:402-425): weight *= ((1*beam)*lik)*extra ; sum ; if sum > 0 normalise and
 * entropy = -sum(w ln w) over w > 0, else weights restored and *restored = 1 (entropy untouched -> NaN here).
 * beam / extra / match_ratio may be NULL (factor 1 / no min-max). */
int mcl3dl_hip_pf_measure(mcl3dl_hip_ctx* ctx, float* weight_inout /*n_p*/, const float* lik /*n_p*/,
                          const float* beam /*n_p or NULL*/, const float* extra /*n_p or NULL*/,
                          const float* match_ratio /*n_p or NULL*/, size_t n_p, float* entropy,
                          float* match_ratio_min, float* match_ratio_max, int* restored);

/* Replaces: the whole `pf_->measure(measure_func)` statement (src/mcl_3dl.cpp:398-426): measure_batch +
 * pf_measure with everything kept on the device in between.  extra = the odometry-error factor
 * NormalLikelihood(odom_err_integ_lin.norm()) computed by the caller (include/mcl_3dl/nd.h:41-58), or NULL.
 * out_lik / out_match_ratio / out_beam may be NULL. */
int mcl3dl_hip_measure_update(mcl3dl_hip_ctx* ctx, const float* pose /*n_p*7*/, const float* extra /*n_p or NULL*/,
                              float* weight_inout /*n_p*/, size_t n_p, const float* scan_lik_xyz, size_t n_s,
                              const float* scan_beam_xyz, const uint32_t* scan_beam_origin, size_t n_b,
                              const float* origins, size_t n_o, float* out_lik, float* out_match_ratio,
                              float* out_beam, float* entropy, float* match_ratio_min, float* match_ratio_max,
                              int* restored);

/* Page-locked host memory for the arrays of the host-buffer entry points. The reference keeps its particles in a
 * std::vector (include/mcl_3dl/pf.h:457) and its scans in pcl::PointCloud objects; a caller that packs poses / scan
 * points for this library anyway can pack them straight into a block from mcl3dl_hip_host_alloc: mcl3dl_hip_measure_update
 * then reads such arrays where they lie (no staging copy, no DMA copy) and writes weight_inout / out_* arrays that lie in
 * such a block directly from the update's last kernel. Arrays anywhere else keep working (staged through the library's
 * own page-locked block). Blocks belong to the context (freed with it); host_free waits for the context's stream. */
int mcl3dl_hip_host_alloc(mcl3dl_hip_ctx* ctx, size_t bytes, void** out);
int mcl3dl_hip_host_free(mcl3dl_hip_ctx* ctx, void* p);

/* Replaces: LidarMeasurementModelBeam::getBeamStatus (src/lidar_measurement_model_beam.cpp:157-192; used for the
 * debug markers at src/mcl_3dl.cpp:471-478) for n explicit rays. hit_index = map index of CastResult::point_
 * (-1 when the ray is exhausted). */
int mcl3dl_hip_beam_status(mcl3dl_hip_ctx* ctx, const float* begin_xyz /*n*3*/, const float* end_xyz /*n*3*/,
                           size_t n, int32_t* status /*n*/, int32_t* hit_index /*n or NULL*/);

/* Replaces: ChunkedKdtree::radiusSearch(p, radius, id, sqdist, 1) (include/mcl_3dl/chunked_kdtree.h:217-237) for n query
 * points (map frame) and ANY radius — besides the likelihood model the node searches with unmatch_output_dist
 * (matched / unmatched clouds, src/mcl_3dl.cpp:776-789) and with the global-localisation grid (:1058-1070).
 * out_index[i] = map index of the nearest point with d2 < (float)(radius*radius) in the dist_weight-rescaled metric, or -1;
 * out_sqdist[i] = that d2 (flann::L2_Simple float arithmetic), -1 when not found. Ties in d2 -> the lowest index. */
int mcl3dl_hip_radius_search(mcl3dl_hip_ctx* ctx, const float* query_xyz /*n*3*/, size_t n, float radius,
                             int32_t* out_index /*n*/, float* out_sqdist /*n or NULL*/);

/* Replaces: driving one RaycastUsingDDA by hand — setRay + getNextCastResult until the first collision
 * (include/mcl_3dl/raycast.h:45-77, include/mcl_3dl/raycasts/raycast_using_dda.h:66-159), the way the reference's
 * waypoint tests do (test/src/test_raycast_dda.cpp:157-183). Uses the caster of mcl3dl_hip_set_beam_params
 * (hit_range = hit_tolerance). out_xyz receives up to max_out voxel centres (CastResult::pos_); *n_visited may exceed
 * max_out. Introspection only: not on the per-update path. */
int mcl3dl_hip_dda_trace(mcl3dl_hip_ctx* ctx, const float* begin3, const float* end3, float* out_xyz /*max_out*3*/,
                         int max_out, int* n_visited, int* collided, int* hit_index);

/* ---- device entry points (asynchronous on the context's stream) ------------------------------------- */
/* Upload (and spatially order) the two filtered scans `pc_locals` of one update (src/mcl_3dl.cpp:377-383). */
int mcl3dl_hip_upload_scan(mcl3dl_hip_ctx* ctx, const float* scan_lik_xyz, size_t n_s, const float* scan_beam_xyz,
                           const uint32_t* scan_beam_origin, size_t n_b, const float* origins, size_t n_o);
/* The order in which the engine holds the likelihood scan it was last given (by mcl3dl_hip_upload_scan, _scan_finish or any
 * host-buffer call): position k holds the caller's point order[k] — a stable sort by the Morton key of 0.25 m cells, which is
 * what gives a wavefront neighbouring points. It matters to a caller in one case: with the option "strict_order" = 3 a
 * particle's likelihood is the reference's float recurrence `score_like += dist * match_weight`
 * (src/lidar_measurement_model_likelihood.cpp:124-134) over the scan IN THIS ORDER, i.e. bit for bit what
 * LidarMeasurementModelLikelihood::measure returns for the cloud { scan[order[0]], scan[order[1]], ... } — computed inside
 * the likelihood kernel, without the N_s x N_p term array and the replay pass that the caller's own order costs
 * ("strict_order" = 1 / 2). The order of a sampled cloud carries no information (PointCloudUniformSampler draws it,
 * include/mcl_3dl/point_cloud_random_samplers/point_cloud_uniform_sampler.h:56-74), but it does select which float
 * roundings happen: two orders of the same points differ by ~1e-6..1e-5 relative, like any two float summation orders. */
int mcl3dl_hip_scan_order(mcl3dl_hip_ctx* ctx, uint32_t* order /*n_s*/, size_t n_s /* must equal the installed scan's size */);
/* The same order computed on the host, without a context or a device (same keys, same stable sort): for a caller that wants
 * to HOLD its sampled cloud in the engine's order — a cloud permuted by `order` is left as it is by the engine (the sort is
 * stable and the keys depend only on the points and their bounding box), so "the caller's order" and "the engine's order"
 * coincide and strict_order = 3 is bit-identical to the reference's measure() on the caller's own cloud. The drop-in model
 * classes do exactly this in filter() when MCL3DL_HIP_ENGINE_ORDER=1. Returns 0, -3 on a null array. */
int mcl3dl_hip_scan_order_host(const float* scan_lik_xyz /*n_s*3*/, size_t n_s, uint32_t* order /*n_s*/);
/* measure_batch on device-resident poses against the uploaded scans; outputs are device arrays (may be NULL). */
int mcl3dl_hip_measure_device(mcl3dl_hip_ctx* ctx, const float* d_pose /*n_p*7*/, size_t n_p, float* d_lik,
                              float* d_match_ratio, float* d_beam);
/* pf::measure split for particle shards (one context per GPU, `world` shards, this one is `rank`):
 *   partial: w_new = w*((1*beam)*lik)*extra kept in the context; d_packed[2 + 2*world] (doubles) = { sum w_new,
 *            sum w_new*ln(w_new), then per rank r: max match_ratio, -min match_ratio } with only THIS rank's pair filled
 *            (the others 0)
 *   [one all-reduce(SUM) of d_packed across the shards — the update's only collective; nothing to do for world == 1]
 *   apply:   weights = w_new / packed[0] if packed[0] > 0, else untouched; d_stats4 = { entropy, match_ratio_min,
 *            match_ratio_max, restored } with entropy = ln S - T/S (== -sum p ln p). */
int mcl3dl_hip_pf_partial_device(mcl3dl_hip_ctx* ctx, const float* d_weight, const float* d_lik, const float* d_beam,
                                 const float* d_extra, const float* d_match_ratio, size_t n_p, int rank, int world,
                                 double* d_packed);
int mcl3dl_hip_pf_apply_device(mcl3dl_hip_ctx* ctx, float* d_weight_inout, size_t n_p, int world,
                               const double* d_packed, float* d_stats4);

/* ---- "next" row: the reductions right after the measurement update ---------------------- */
/* Replaces: pf::ParticleFilter::expectationBiased (include/mcl_3dl/pf.h:294-303, called at src/mcl_3dl.cpp:451) with
 * ParticleWeightedMeanQuat (include/mcl_3dl/state_6dof.h:316-355), and max() / maxBiased() (pf.h:361-390, :452).
 * bias NULL = probability_bias_ 1 (= expectation over all particles). out_mean7 = px,py,pz,qx,qy,qz,qw;
 * out_total = sum of weight*bias; the max indices are those of the FIRST maximum (strict < in the reference).
 * Per-particle products are the reference's float expressions; sums are fp64 trees (reference: float sequential). */
int mcl3dl_hip_expectation(mcl3dl_hip_ctx* ctx, const float* pose /*n*7*/, const float* weight /*n*/,
                           const float* bias /*n or NULL*/, size_t n, float* out_mean7, float* out_total,
                           int32_t* out_max_index, int32_t* out_max_biased_index);
/* Replaces: pf::ParticleFilter::covariance (pf.h:304-360, called at src/mcl_3dl.cpp:373,706) with
 * State6DOF::covElement (state_6dof.h:162-184) about `mean7` (the caller's expectation). subset = the particle indices
 * the caller's RNG drew for random_sample_ratio < 1 (pf.h:322-336), or NULL = all n particles. out_cov36 row-major. */
int mcl3dl_hip_covariance(mcl3dl_hip_ctx* ctx, const float* pose /*n*7*/, const float* weight /*n*/, size_t n,
                          const uint32_t* subset /*n_subset or NULL*/, size_t n_subset, const float* mean7,
                          float* out_cov36);
/* The same on device-resident poses / weights (results still returned to the host: they are a dozen scalars). */
int mcl3dl_hip_expectation_device(mcl3dl_hip_ctx* ctx, const float* d_pose, const float* d_weight, const float* d_bias,
                                  size_t n, float* out_mean7, float* out_total, int32_t* out_max_index,
                                  int32_t* out_max_biased_index);
int mcl3dl_hip_covariance_device(mcl3dl_hip_ctx* ctx, const float* d_pose, const float* d_weight, size_t n_particles,
                                 const uint32_t* d_subset, size_t n_subset, const float* mean7, float* out_cov36);

/* The same reductions over particle shards (multi-GPU hosts, mcl_3dl_amd/distributed.py:sharded_expectation /
 * sharded_covariance). *_partial_device leaves one record per shard in DEVICE memory:
 *   moments    16 doubles {sum w, sum w*pos[3], sum w*front[3], sum w*up[3], max w, its index in the shard,
 *              max w*bias, its index, 0, 0}      -> all-gather, then mcl3dl_hip_moments_finish (host arithmetic of
 *              ParticleWeightedMeanQuat::getMean, state_6dof.h:345-350; index_offset[r] = first particle of shard r)
 *   covariance 22 doubles {21 upper-triangular sums, sum w} -> all-reduce(SUM), then mcl3dl_hip_covariance_finish.
 * An empty shard (n == 0; its particle arrays may be NULL) is no error for either *_partial_device: its covariance record is
 * 22 zeros, its moments record ten zero sums with both maxima at -1 (indices 0), which mcl3dl_hip_moments_finish never picks.
 * (mcl3dl_hip_expectation_device / _covariance_device, which divide by the sum, keep rejecting n == 0.)
 * The *_finish functions are pure host functions (no context). */
int mcl3dl_hip_moments_partial_device(mcl3dl_hip_ctx* ctx, const float* d_pose, const float* d_weight,
                                      const float* d_bias /*or NULL*/, size_t n, double* d_out16);
int mcl3dl_hip_moments_finish(const double* parts16 /*world*16, rank order*/, int world,
                              const uint64_t* index_offset /*world or NULL*/, float* out_mean7, float* out_total,
                              int64_t* out_max_index, int64_t* out_max_biased_index);
int mcl3dl_hip_covariance_partial_device(mcl3dl_hip_ctx* ctx, const float* d_pose, const float* d_weight,
                                         size_t n_particles, const uint32_t* d_subset /*or NULL*/, size_t n_subset,
                                         const float* mean7 /*host*/, double* d_out22);
int mcl3dl_hip_covariance_finish(const double* sums22, float* out_cov36);

/* ---- "next" row: resampling ------------------------------------------------------------------ */
/* Replaces: pf::ParticleFilter::resample (include/mcl_3dl/pf.h:187-225, called at src/mcl_3dl.cpp:809) and
 * resizeParticle (pf.h:399-436, :880-884) on 13-dof states (State6DOF::operator[], state_6dof.h:80-149: pos, rot,
 * odom_err_integ_lin, odom_err_integ_ang). The caller keeps its random engine, so the sequence is three calls:
 *   begin : float prefix sums of the weights + the std::sort of the duplicate array (tie groups of weight-0 particles
 *           are ordered by libstdc++'s introsort exactly as in the reference); returns pstep = accum / n_out
 *   [resample only: the caller draws initial_p = uniform_real_distribution<float>(0, pstep)(engine_), pf.h:203]
 *   plan  : mode 0 = resample (pscan = pstep*i + initial_p), 1 = resizeParticle (pscan += pstep; initial_p ignored);
 *           n_out lower_bound searches on the device; out_source[i] = particle copied into slot i,
 *           out_duplicate[i] = 1 where the reference adds noise (it == it_prev, pf.h:217-221)
 *   [the caller draws one State6DOF::generateNoise per duplicated slot, in slot order, pf.h:216]
 *   apply : gather on the device; duplicated slots get state + noise (State6DOF::operator+, state_6dof.h:248-260)
 *           and normalize() (:150-153). New weights are 1/n_out (pf.h:207 / 419) — the caller's to set.
 * any out_* may be NULL. noise13 holds n_noise >= (number of duplicates) 13-float noise states. */
int mcl3dl_hip_resample_begin(mcl3dl_hip_ctx* ctx, const float* weight /*n*/, size_t n, size_t n_out, float* out_pstep);
int mcl3dl_hip_resample_plan(mcl3dl_hip_ctx* ctx, int mode, float initial_p, uint32_t* out_source /*n_out*/,
                             uint8_t* out_duplicate /*n_out*/, size_t* out_n_duplicates);
int mcl3dl_hip_resample_apply(mcl3dl_hip_ctx* ctx, const float* state13_in /*n*13*/, const float* noise13, size_t n_noise,
                              float* state13_out /*n_out*13*/);
int mcl3dl_hip_resample_apply_device(mcl3dl_hip_ctx* ctx, const float* d_state13_in, const float* noise13 /*host*/,
                                     size_t n_noise, float* d_state13_out);
/* Device-resident / sharded variants. begin_device takes the weights from device memory (they travel to the host: the
 * prefix sums are a sequential float recurrence). apply_slice_device fills only the output slots
 * [out_begin, out_begin + out_count) — a rank's own shard when particles are split over GPUs: every rank plans on the
 * all-gathered weights, gathers the states, and writes its slice (mcl_3dl_amd/distributed.py:sharded_resample).
 * d_state13_in holds all n input particles, d_state13_out out_count states, noise13 the noise of ALL duplicated slots. */
int mcl3dl_hip_resample_begin_device(mcl3dl_hip_ctx* ctx, const float* d_weight /*n*/, size_t n, size_t n_out,
                                     float* out_pstep);
int mcl3dl_hip_resample_apply_slice_device(mcl3dl_hip_ctx* ctx, const float* d_state13_in, const float* noise13 /*host*/,
                                           size_t n_noise, size_t out_begin, size_t out_count, float* d_state13_out);

/* One device-resident update in one call (single GPU): measure_device + pf_partial_device + pf_apply_device, i.e. the
 * statement pf_->measure(measure_func) of src/mcl_3dl.cpp:398-426 on device arrays. d_extra, d_lik, d_match_ratio,
 * d_beam may be NULL (no odometry factor / results kept internally); d_stats4 as in pf_apply_device.
 * Results are identical to the three separate calls. (Until ABI 2 an option "use_graph" replayed the sequence from a
 * captured hipGraph; on ROCm 7.2 / MI355X a replay cost a fixed 10-16 us against 3.3-3.8 us per plain launch and measured
 * slower at every size, so the option and its two introspection calls are gone in ABI 3.) */
int mcl3dl_hip_update_device(mcl3dl_hip_ctx* ctx, const float* d_pose, size_t n_p, float* d_weight_inout,
                             const float* d_extra, float* d_lik, float* d_match_ratio, float* d_beam, float* d_stats4);

/* ---- "next" row: scan preparation on the GPU ------------------------------------------------------
 * Replaces, for one measurement update: the pcl::VoxelGrid down-sampling of the accumulated cloud
 * (src/mcl_3dl.cpp:363-367), both models' clip filter (src/lidar_measurement_model_likelihood.cpp:79-103,
 * src/lidar_measurement_model_beam.cpp:98-122) and the sampler's gather
 * (include/mcl_3dl/point_cloud_random_samplers/point_cloud_uniform_sampler.h:56-74) — the random engine stays with the
 * caller, like resampling:
 *   begin  : cloud (robot frame; label = index of the accumulated cloud, src/mcl_3dl.cpp:295-298) -> VoxelGrid(leaf3;
 *            a component <= 0 or NULL skips it) -> pc_local_full; clipped copies for the likelihood and the beam model
 *            (clip = {clip_near, clip_far, clip_z_min, clip_z_max}; NULL = that model is not used). Returns the three
 *            sizes; the clouds stay on the device.
 *   [the caller draws n_s resp. n_b indices with std::uniform_int_distribution<size_t>(0, size - 1), sampler.h:66-71]
 *   finish : gathers the drawn points, orders them (the ordering mcl3dl_hip_upload_scan does on the host, same keys, same
 *            stable order) and installs them as the scans of the next mcl3dl_hip_measure_device / _update_device — no
 *            host round trip of the points. Results are bit-identical to uploading the same sampled clouds.
 * VoxelGrid follows pcl::VoxelGrid<PointXYZIL> as the node configures it (setLeafSize only): leaf index
 * int(floor(p * inv_leaf) - float(min_b)) . divb_mul, one centroid per occupied leaf in ascending leaf order, label = the
 * most frequent one (smallest on a tie); xyz are summed as floats in INPUT order (PCL's own std::sort leaves the order
 * inside a leaf unspecified; PCL is not vendored by the reference: parity at this boundary is against the restatement
 * in oracle/). Non-finite points are dropped by the filter. Intensity is not carried.
 * download: which = 0 pc_local_full, 1 / 2 clipped likelihood / beam cloud, 3 / 4 sampled clouds in the caller's index
 * order (xyz NULL: only *n); 5 / 6 the likelihood / beam scan AS INSTALLED, in the engine's order (n_s points, label 0 /
 * n_b points, label = origin id) — available whenever a scan is installed, by mcl3dl_hip_upload_scan (ordered on the host
 * or on the device), _scan_finish or a host-buffer update call; 0..4 need a mcl3dl_hip_scan_begin. */
int mcl3dl_hip_scan_begin(mcl3dl_hip_ctx* ctx, const float* xyz /*n*3*/, const uint32_t* label /*n or NULL*/, size_t n,
                          const float* leaf3, const float* clip_lik4, const float* clip_beam4, size_t* n_full,
                          size_t* n_lik_clipped, size_t* n_beam_clipped);
/* The same from the wire format (mcl_3dl::fromROSMsg, include/mcl_3dl/point_conversion.h:64-92): little-endian
 * sensor_msgs/PointCloud2 data with FLOAT32 x / y / z at the given byte offsets and an optional UINT32 "label" field
 * (off_label < 0: none). label_override = 0 stamps every point with accumulated-cloud index 0 (what accumCloud does for
 * the first / only cloud), 0xffffffff keeps the message's labels.
 * LAYOUT REQUIRED by every *_pointcloud2 entry point: `data` is n_points * point_step bytes, i.e. rows without padding
 * (row_step == width * point_step), is_bigendian == false, and x / y / z (label) of datatype FLOAT32 (UINT32). The
 * reference's pcl::fromROSMsg also takes padded rows and big-endian data; a caller holding such a message checks it with
 * mcl3dl_hip_pointcloud2_layout_ok() below and repacks it (or passes plain arrays) when that returns 0 — the entry points
 * cannot see width / row_step / endianness and would decode shifted points without an error. */
static inline int mcl3dl_hip_pointcloud2_layout_ok(uint32_t width, uint32_t height, uint32_t point_step, uint32_t row_step,
                                                   int is_bigendian, int datatype_x, int datatype_y, int datatype_z,
                                                   int datatype_label /* -1: no label field */)
{
  /* sensor_msgs/PointField: FLOAT32 = 7, UINT32 = 6 */
  return !is_bigendian && (height <= 1 || row_step == width * point_step) && datatype_x == 7 && datatype_y == 7 &&
         datatype_z == 7 && (datatype_label < 0 || datatype_label == 6);
}
int mcl3dl_hip_scan_begin_pointcloud2(mcl3dl_hip_ctx* ctx, const uint8_t* data, size_t n_points, uint32_t point_step,
                                      int off_x, int off_y, int off_z, int off_label, uint32_t label_override,
                                      const float* leaf3, const float* clip_lik4, const float* clip_beam4, size_t* n_full,
                                      size_t* n_lik_clipped, size_t* n_beam_clipped);
int mcl3dl_hip_scan_finish(mcl3dl_hip_ctx* ctx, const uint32_t* idx_lik /*n_s*/, size_t n_s,
                           const uint32_t* idx_beam /*n_b*/, size_t n_b, const float* origins /*n_o*3*/, size_t n_o);
int mcl3dl_hip_scan_download(mcl3dl_hip_ctx* ctx, int which, float* xyz, uint32_t* label, size_t capacity, size_t* n);
/* Introspection: the stable radix sort the cloud path runs on the device (VoxelGrid leaf order, scan ordering; replaces the
 * std::sort of pcl::VoxelGrid and nothing else of the reference), exposed so that it can be checked on its own:
 * (keys, vals) sorted ascending by key bits [0, end_bit), equal keys in input order. One launch up to 2048 pairs. */
int mcl3dl_hip_sort_pairs(mcl3dl_hip_ctx* ctx, const uint32_t* keys, const uint32_t* vals /*NULL: 0..n-1*/, size_t n,
                          int end_bit, uint32_t* out_keys, uint32_t* out_vals);

/* ---- "next" row: map from the wire format, map updates, matched / unmatched output --------------
 * set_map_*: replaces cbMapcloud + loadMapCloud (src/mcl_3dl.cpp:128-139, 1140-1158): decode, VoxelGrid(map_downsample),
 * then as mcl3dl_hip_set_map. *n_map = points kept.
 * map_update*: replaces cbMapcloudUpdate + cbMapUpdateTimer (src/mcl_3dl.cpp:141-153, 1355-1369): pc_map2 = pc_map +
 * VoxelGrid(update, update_downsample); a later update REPLACES the earlier one (n = 0 removes it). The candidate-voxel
 * index is not rebuilt: only the bricks within reach of a removed or an added point are compiled again (from the points
 * that can reach them) and installed over their old records — results identical to a fresh index of the merged map.
 * stats6 (may be NULL) = {bricks re-compiled, bricks added, points that took part, device milliseconds, overflow
 * records appended, outcome}; outcome 0 = incremental update done; otherwise the index is rebuilt as a whole on next use:
 * 1 nothing was built yet, 2 lik_index != 2, 3 the index was built for another point count, 4 a point outside the grid
 * the index was laid out for, 5 brick / overflow budget exhausted; 6 = no brick touched (nothing to do).
 * map_download: the map as the engine holds it (base, then update). */
int mcl3dl_hip_set_map_pointcloud2(mcl3dl_hip_ctx* ctx, const uint8_t* data, size_t n_points, uint32_t point_step, int off_x,
                                   int off_y, int off_z, int off_label, const float* leaf3, uint64_t stamp,
                                   const float* dist_weight, size_t* n_map);
int mcl3dl_hip_set_map_downsampled(mcl3dl_hip_ctx* ctx, const float* xyz, const uint32_t* label, size_t n,
                                   const float* leaf3, uint64_t stamp, const float* dist_weight, size_t* n_map);
int mcl3dl_hip_map_update(mcl3dl_hip_ctx* ctx, const float* xyz, const uint32_t* label, size_t n, const float* leaf3,
                          uint64_t stamp, size_t* n_map, double* stats6);
int mcl3dl_hip_map_update_pointcloud2(mcl3dl_hip_ctx* ctx, const uint8_t* data, size_t n_points, uint32_t point_step,
                                      int off_x, int off_y, int off_z, int off_label, const float* leaf3, uint64_t stamp,
                                      size_t* n_map, double* stats6);
int mcl3dl_hip_map_download(mcl3dl_hip_ctx* ctx, float* xyz, uint32_t* label, size_t capacity, size_t* n);
/* Replaces the matched / unmatched classification of src/mcl_3dl.cpp:761-805 as ONE device pass: every point of
 * pc_local_full (xyz NULL: the cloud mcl3dl_hip_scan_begin left on the device; otherwise n explicit robot-frame points)
 * is transformed by the pose (State6DOF::transform), searched with radiusSearch(p, unmatch_dist, ., ., 1); no neighbour ->
 * unmatched; sqdist < match_dist^2 (compared in double, :778-786) -> matched. Outputs are the transformed points in input
 * order (NULL: counts only). */
int mcl3dl_hip_match_split(mcl3dl_hip_ctx* ctx, const float* pose7, const float* xyz, size_t n, float unmatch_dist,
                           double match_dist, float* out_matched_xyz, size_t cap_matched, size_t* n_matched,
                           float* out_unmatched_xyz, size_t cap_unmatched, size_t* n_unmatched);

/* ---- device groups: N GPUs behind one handle, one host process ----------------------------------
 * The reference node is ONE C++ process (src/mcl_3dl.cpp:1466); a group lets that process use every GPU of the node with
 * src/mcl_3dl.cpp untouched: the drop-in model classes call the group_* forms of the entry points above.
 * A group owns one context per listed device and one worker thread per device. Particles are split into contiguous
 * shards (mcl3dl_hip_group_shard: sizes differ by at most one), map / parameters / scan are replicated on every device,
 * and one update needs exactly ONE collective — the all-reduce(sum) of the 2 + 2N doubles described at
 * mcl3dl_hip_pf_partial_device:
 *   "collective" 0 (default): ncclAllReduce on each device's stream (RCCL over xGMI; librccl is dlopen'ed the first time
 *                a group of more than one device runs an update — MCL3DL_HIP_RCCL_LIB overrides the library name)
 *   "collective" 1 (or environment MCL3DL_HIP_COLLECTIVE=host): the N records are brought to the host, summed in rank
 *                order and sent back — for several contexts on ONE GPU (RCCL needs one GPU per rank) and as a fallback.
 * With one device every group_* call is the plain call on its context (bit-identical results, no thread, no RCCL);
 * option "direct_single" = 0 sends a one-device group through the sharded path as well (tests: RCCL with one rank).
 * A group is not thread-safe (one caller at a time), like a context. */
typedef struct mcl3dl_hip_group mcl3dl_hip_group;
int mcl3dl_hip_group_create(mcl3dl_hip_group** out, const int* device_ids, int n_devices /* 1..64 */);
void mcl3dl_hip_group_destroy(mcl3dl_hip_group* g);
const char* mcl3dl_hip_group_last_error(const mcl3dl_hip_group* g);
int mcl3dl_hip_group_size(const mcl3dl_hip_group* g);
/* The context of one rank (options, introspection, per-device queries such as mcl3dl_hip_beam_status). */
mcl3dl_hip_ctx* mcl3dl_hip_group_context(mcl3dl_hip_group* g, int rank);
/* Shard bookkeeping (pure host function): particles [*begin, *begin + *count) belong to `rank`. */
int mcl3dl_hip_group_shard(size_t n_p, int n_devices, int rank, size_t* begin, size_t* count);
/* Broadcast forms of mcl3dl_hip_set_map / _set_likelihood_params / _set_beam_params / _set_option
 * ("collective" is the group's own option, everything else goes to every context). */
int mcl3dl_hip_group_set_map(mcl3dl_hip_group* g, const float* xyz, const uint32_t* label, size_t n_m, uint64_t stamp,
                             const float* dist_weight);
int mcl3dl_hip_group_set_likelihood_params(mcl3dl_hip_group* g, float match_dist_min, float match_dist_flat,
                                           float match_weight);
int mcl3dl_hip_group_set_beam_params(mcl3dl_hip_group* g, float map_grid_x, float map_grid_y, float map_grid_z,
                                     float dda_grid_size, float ray_angle_half, float hit_range,
                                     float beam_likelihood_min, uint32_t num_points, float ang_total_ref,
                                     uint32_t filter_label_max, int add_penalty_short_only_mode);
/* Replaces: beam/use_raycast_using_dda (src/parameters.cpp:289) for every rank's model at once: mcl3dl_hip_set_beam_raycast
 * on every context of the group. */
int mcl3dl_hip_group_set_beam_raycast(mcl3dl_hip_group* g, int mode);
int mcl3dl_hip_group_set_option(mcl3dl_hip_group* g, const char* name, double value);
/* Sharded forms of mcl3dl_hip_upload_poses / _measure_batch / _measure_update: same arguments, same results; host arrays
 * are scattered to / gathered from the shards. measure_batch needs no collective; measure_update runs the one all-reduce. */
int mcl3dl_hip_group_upload_poses(mcl3dl_hip_group* g, const float* pose /*n_p*7*/, size_t n_p);
int mcl3dl_hip_group_measure_batch(mcl3dl_hip_group* g, const float* pose /*n_p*7 or NULL*/, size_t n_p,
                                   const float* scan_lik_xyz, size_t n_s, const float* scan_beam_xyz,
                                   const uint32_t* scan_beam_origin, size_t n_b, const float* origins, size_t n_o,
                                   float* out_lik, float* out_match_ratio, float* out_beam);
/* mcl3dl_hip_measure_batch_begin / _wait / _end for a group: one device delivers slice by slice; a sharded group evaluates
 * the whole batch inside _begin and _wait reports every particle ready. */
int mcl3dl_hip_group_measure_batch_begin(mcl3dl_hip_group* g, const float* pose /*n_p*7 or NULL*/, size_t n_p,
                                         const float* scan_lik_xyz, size_t n_s, const float* scan_beam_xyz,
                                         const uint32_t* scan_beam_origin, size_t n_b, const float* origins, size_t n_o,
                                         float* out_lik, float* out_match_ratio, float* out_beam, size_t slice_particles);
int mcl3dl_hip_group_measure_batch_wait(mcl3dl_hip_group* g, size_t particle, size_t* n_ready);
int mcl3dl_hip_group_measure_batch_end(mcl3dl_hip_group* g);
int mcl3dl_hip_group_measure_update(mcl3dl_hip_group* g, const float* pose, const float* extra, float* weight_inout,
                                    size_t n_p, const float* scan_lik_xyz, size_t n_s, const float* scan_beam_xyz,
                                    const uint32_t* scan_beam_origin, size_t n_b, const float* origins, size_t n_o,
                                    float* out_lik, float* out_match_ratio, float* out_beam, float* entropy,
                                    float* match_ratio_min, float* match_ratio_max, int* restored);
/* ---- the group's particles RESIDENT on its GPUs: a whole filter iteration without a per-update pose upload ----------------
 * Replaces, for N GPUs, what the node does with pf_ around the measurement (src/mcl_3dl.cpp:398-452, 706-709, 809):
 *   upload_state      the particle vector (include/mcl_3dl/pf.h:457) as 13 floats per particle {pos 3, rot 4 (x,y,z,w),
 *                     odom_err_integ lin 3, ang 3} (State6DOF, state_6dof.h:56-66) + probabilities (NULL: 1 / n_p each),
 *                     scattered into contiguous shards (mcl3dl_hip_group_shard); they stay on the devices until the next
 *                     upload. What the node does to the particles between two scans (motion prediction, IMU measurement,
 *                     odometry noise, the odometry-error reset) runs on the resident particles too: see the calls below.
 *   update_resident   pf::measure (pf.h:252-279 with the lambda of src/mcl_3dl.cpp:402-425) over the resident particles:
 *                     only the scan (and the odometry factor `extra`, n_p floats or NULL) goes up, one all-reduce of
 *                     2 + 2N doubles, four scalars come back; out_weight / out_lik / out_match_ratio / out_beam (each may be
 *                     NULL) fetch per-particle results. Same results as mcl3dl_hip_group_measure_update on the same particles.
 *   expectation       pf::expectationBiased + max + maxBiased (pf.h:294-303, 361-390): one 16-double record per shard,
 *                     combined on the host (mcl3dl_hip_moments_finish); bias = probability_bias_ per particle or NULL.
 *   covariance        pf::covariance about mean7 (pf.h:304-360, all particles): 22 sums per shard, added in rank order.
 *   resample_begin    accum_probability_ (pf.h:193-197 / 401-405): the float recurrence is sequential over ALL particles, so
 *                     every weight comes to the host once (4 B per particle) and the prefixes go to every device; n_out = 0
 *                     keeps the particle count (resample), another value is resizeParticle (pf.h:399-436). *out_pstep for
 *                     the caller's uniform draw (pf.h:203).
 *   resample_plan     mode / initial_p / outputs as mcl3dl_hip_resample_plan (every rank plans all slots: n_out searches).
 *   resample_apply    all-gather of the 13-float states (ncclAllGather over xGMI; through the host with "collective" 1), every
 *                     rank writes ITS shard of the new generation (duplicates get noise13[slot], State6DOF::operator+ and
 *                     normalize(): pf.h:214-218), weights 1 / n_out (pf.h:207), poses refreshed. The particles are resident
 *                     again, n_out of them.
 * With one device and "direct_single" 1 none of this touches RCCL. */
int mcl3dl_hip_group_upload_state(mcl3dl_hip_group* g, const float* state13 /*n_p*13*/, const float* weight /*n_p or NULL*/,
                                  size_t n_p);
int mcl3dl_hip_group_download_state(mcl3dl_hip_group* g, float* state13 /*n_p*13 or NULL*/, float* weight /*n_p or NULL*/,
                                    size_t n_p);
size_t mcl3dl_hip_group_resident(const mcl3dl_hip_group* g);
int mcl3dl_hip_group_update_resident(mcl3dl_hip_group* g, const float* extra /*n_p or NULL*/, const float* scan_lik_xyz,
                                     size_t n_s, const float* scan_beam_xyz, const uint32_t* scan_beam_origin, size_t n_b,
                                     const float* origins, size_t n_o, float* out_weight, float* out_lik,
                                     float* out_match_ratio, float* out_beam, float* entropy, float* match_ratio_min,
                                     float* match_ratio_max, int* restored);
int mcl3dl_hip_group_expectation(mcl3dl_hip_group* g, const float* bias /*n_p or NULL*/, float* out_mean7, float* out_total,
                                 int64_t* out_max_index, int64_t* out_max_biased_index);
int mcl3dl_hip_group_covariance(mcl3dl_hip_group* g, const float* mean7, float* out_cov36);
/* The pose-jump bias of every scan + the biased expectation, in one pass over the resident particles.
 * Replaces pf_->bias(bias_func) + expectationBiased() + max() of src/mcl_3dl.cpp:436-452 (the branch for at most num_particles_
 * particles; the uniform-bias branch :428-435 is mcl3dl_hip_group_expectation with bias == NULL):
 *   probability_bias_ = nl_lin(|pos - prev.pos|) * nl_ang(ang) + 1e-6 with NormalLikelihood<float>(bias_var_dist / bias_var_ang)
 *   (nd.h:41-58; the two values are used as sigmas, as the reference does) and ang = getAxisAng (quat.h:226-239) of
 *   rot * prev.rot.inv(), formed from each RESIDENT pose inside the moments pass of mcl3dl_hip_group_expectation: no bias array
 *   exists unless out_bias (n_p floats) asks for it. Mean, total, max and biased-max index are those of
 *   mcl3dl_hip_group_expectation(g, <these biases>, ...), bit for bit. prev7 = state_prev_ {pos 3, rot x, y, z, w}.
 * -3: a NULL or non-finite prev7, a sigma that is not finite and > 0. -5: no resident particles.
 *   download_particle   pf_->max()'s STATE (src/mcl_3dl.cpp:452): the 13 floats and the weight of ONE resident particle, copied
 *                       from the rank that owns it (mcl3dl_hip_group_shard), no collective. Either output may be NULL.
 *                       -3: index out of range. */
int mcl3dl_hip_group_expectation_jump_bias(mcl3dl_hip_group* g, const float* prev7, float bias_var_dist, float bias_var_ang,
                                           float* out_bias /*n_p or NULL*/, float* out_mean7, float* out_total,
                                           int64_t* out_max_index, int64_t* out_max_biased_index);
int mcl3dl_hip_group_download_particle(mcl3dl_hip_group* g, int64_t index, float* out_state13, float* out_weight);
int mcl3dl_hip_group_resample_begin(mcl3dl_hip_group* g, size_t n_out /*0 = as many as there are*/, float* out_pstep);
int mcl3dl_hip_group_resample_plan(mcl3dl_hip_group* g, int mode, float initial_p, uint32_t* out_source /*n_out or NULL*/,
                                   uint8_t* out_duplicate /*n_out or NULL*/, size_t* out_n_duplicates);
int mcl3dl_hip_group_resample_apply(mcl3dl_hip_group* g, const float* noise13 /*n_dup*13, host*/, size_t n_noise);
/* ---- between two scans, on the resident particles (no state download) --------------------------------------------------
 * The rest of what src/mcl_3dl.cpp does to every particle. All but measure_imu / measure_landmark are shard-local: one launch per device, no
 * collective. The caller keeps drawing the random numbers (the reference draws them from one sequential engine), as for
 * resample_apply's noise13.
 *   set_odom_noise       State6DOF's odometry noise {noise_ll_, noise_la_, noise_al_, noise_aa_} per resident particle, already
 *                        scaled by the caller (src/mcl_3dl.cpp:817-825 draws N(0, 1) * odom_err_*). upload_state installs zeros
 *                        (State6DOF's constructors); resample_apply keeps a copied particle's noise and gives a duplicated one
 *                        zeros (pf.h:211-222: operator+ returns a fresh State6DOF); add_noise zeroes it. download_odom_noise
 *                        reads it back.
 *   predict              cbOdom (src/mcl_3dl.cpp:227-232): MotionPredictionModelDifferentialDrive(lin_tc, ang_tc)
 *                        (motion_prediction_model_differential_drive.h:46-67): setOdoms(prev, cur, time_diff) on the host, predict()
 *                        on every particle. Poses are 7 floats {pos 3, rot x, y, z, w}.
 *   reset_odom_integ     integ_reset_func (src/mcl_3dl.cpp:190-195, 652-658): odom_err_integ_lin_ = odom_err_integ_ang_ = 0.
 *   add_noise            pf::noise / addNoiseUsingNoiseGenerator (pf.h:226-237, the expansion reset of src/mcl_3dl.cpp:850-860):
 *                        state = state + noise13[i] (State6DOF::operator+, state_6dof.h:249-260), noise caller-drawn.
 *   measure_imu          cbImu (src/mcl_3dl.cpp:997-1002): pf::measure (pf.h:252-279) with ImuMeasurementModelGravity(acc_var)
 *                        after setAccMeasure(acc3) (imu_measurement_model_gravity.h:41-56); the same partial sums, all-reduce
 *                        and restore rule as update_resident. out_weight / out_lik may be NULL.
 *   set_odom_error_sigma measure()'s odometry factor (src/mcl_3dl.cpp:420-423): sigma > 0 makes update_resident with extra == NULL
 *                        apply NormalLikelihood(sigma)(|odom_err_integ_lin_|) formed on the devices from the resident states;
 *                        0 (the default) keeps NULL's meaning, no factor.
 *   measure_landmark     cbLandmark (src/mcl_3dl.cpp:899-929): pf::measure with NormalLikelihoodNd<float, 6> (nd.h:60-80) over
 *                        {pos, getRPY(rot)} of s - measured (state_6dof.h:262-274, quat.h:191-201); the odometry-error fields
 *                        take no part. measured7 = {pos 3, rot x, y, z, w}. cov36 is the message's covariance array as the
 *                        reference maps it: COLUMN-major, sigma(r, c) = (float)cov36[6 * c + r] (moot for a symmetric matrix).
 *                        Determinant and inverse of the float matrix come from an LU with partial pivoting in double, each
 *                        rounded to float once; x^T sigma^-1 x is summed sequentially in float (Eigen's own LU and reduction
 *                        order are not pinned by the reference: DESIGN.md). A launch of its own forms the likelihoods, then the
 *                        same partial sums, all-reduce and restore rule as measure_imu. -3: NULL or non-finite arguments, a
 *                        singular covariance or one without a positive determinant (the reference would weigh with NaN and
 *                        restore). A determinant beyond float range is no error: a_ = 0, every likelihood 0, the update
 *                        restores, as in the reference. The caller resamples afterwards (resample_begin / _plan / _apply).
 * sinf / cosf / acosf / expf / atan2f / asinf of the reference are evaluated in double and rounded to float on the device
 * (within 1 ulp of a faithful libm; DESIGN.md, "Numerics"); everything else is the reference's float arithmetic in its order. */
int mcl3dl_hip_group_set_odom_noise(mcl3dl_hip_group* g, const float* noise4 /*n_p*4*/, size_t n_p);
int mcl3dl_hip_group_download_odom_noise(mcl3dl_hip_group* g, float* noise4 /*n_p*4*/, size_t n_p);
int mcl3dl_hip_group_predict(mcl3dl_hip_group* g, const float* odom_prev7, const float* odom_cur7, float time_diff,
                             float odom_err_integ_lin_tc, float odom_err_integ_ang_tc);
int mcl3dl_hip_group_reset_odom_integ(mcl3dl_hip_group* g);
int mcl3dl_hip_group_add_noise(mcl3dl_hip_group* g, const float* noise13 /*n_p*13*/, size_t n_p);
int mcl3dl_hip_group_measure_imu(mcl3dl_hip_group* g, const float* acc3, float acc_var, float* out_weight /*n_p or NULL*/,
                                 float* out_lik /*n_p or NULL*/, float* entropy, int* restored);
int mcl3dl_hip_group_set_odom_error_sigma(mcl3dl_hip_group* g, float sigma);
/* ---- the noise drawn on the devices, from the reference's engine ---------------------------------------------------------
 * The draws above (noise13 of resample_apply and add_noise, noise4 of set_odom_noise) and pf::init, without the host drawing or
 * uploading anything: std::default_random_engine as libstdc++ defines it (minstd_rand0, x <- 16807 x mod (2^31 - 1); the
 * library the reference oracle is built with: another standard library uses another engine) and its
 * normal_distribution<float>, evaluated for every position of the stream at once. engine_state is in / out:
 * the engine's state in [1, 2^31 - 2]; behind a call it holds what the reference's engine_ would hold, so any mix of these
 * calls with the caller's own draws stays on the reference's stream. A std::default_random_engine gives and takes its state
 * through operator<< / operator>>. The logarithm of the polar method is taken in double and rounded to float (the rule above for
 * the transcendentals): accept / reject decisions and the engine state are the reference's exactly, the values are within
 * 1 ulp-of-log of a faithful logf.
 *   rng_seed              engine(seed)'s state. Host only.
 *   rng_uniform           uniform_real_distribution<float>(a, b)(engine), pf::resample's initial_p (pf.h:199): one engine call.
 *                         Host only. NaN for a NULL state or one outside [1, 2^31 - 2].
 *   add_noise_drawn       add_noise with generateNoise(engine, DiagonalNoiseGenerator(State6DOF(), sigma6)) per particle
 *                         (sigma6 = {x, y, z, roll, pitch, yaw}; a zero sigma draws nothing, diagonal_noise_generator.h:69-73).
 *   init_drawn            pf::init(mean, sigma) (pf.h:169-181): n_p states generateNoise(engine, DiagonalNoiseGenerator(mean7,
 *                         sigma6)), weights 1 / n_p; the particles become resident as after upload_state. mean7 = {pos 3, rot
 *                         x, y, z, w}; its getRPY is formed once on the host.
 *   draw_odom_noise       set_odom_noise with update_noise_func's draws (src/mcl_3dl.cpp:817-825): ONE normal_distribution<float>
 *                         (0, 1) per call, four values per particle in the order ll, la, aa, al, each times its odom_err4 entry
 *                         {lin_lin, lin_ang, ang_ang, ang_lin}.
 *   resample_apply_drawn  resample_apply with generateNoise per duplicated slot in slot order (pf.h:216); duplicated particles
 *                         get zero odometry noise, as there.
 *   noise_transform6      MultivariateNoiseGenerator::setCovariance (multivariate_noise_generator.h:63-77) for the `initialpose`
 *                         covariance: transform36 = V diag(sqrt(lambda)), row-major 6x6. Host only. A definition of this
 *                         library's own: the 36 doubles cast to float, the lower triangle read, a cyclic Jacobi in double (30
 *                         sweeps at the most), eigenvalues ascending, each eigenvector's largest component positive (lowest index
 *                         on a tie), T[i][k] = (float)(V[i][k] sqrt(lambda_k)). No Eigen release's eigenvectors are reproduced
 *                         (within a repeated eigenvalue any orthonormal basis is valid): particles drawn with it have the
 *                         reference's distribution, not its bits. An eigenvalue in [-2^-23 |C|_F, 0) — what rounding a positive
 *                         semi-definite matrix to float can produce — is set to 0; -3 for a more negative one (the reference
 *                         would fill the particles with NaN; the message on stderr names the eigenvalue), for NULL cov36 /
 *                         transform36 and for a non-finite entry. eigenvalues6 may be NULL.
 *   init_drawn_multivariate  cbPosition (src/mcl_3dl.cpp:186-195): pf_->initUsingNoiseGenerator(MultivariateNoiseGenerator<float>(
 *                         mean, cov)) and, with reset_odom_integ = 1, the integ_reset_func pass behind it. Per particle ONE
 *                         normal_distribution<float>(0, 1) is called six times (multivariate_noise_generator.h:80-91): 3 n_p
 *                         accepted attempts of one shared stream, then org = mean6 + transform36 * values in float, the six
 *                         products summed left to right without fused multiply-add (Eigen's association is not pinned), and
 *                         generateNoise as for init_drawn; weights 1 / n_p, odometry noise 0. It takes the transform, not the
 *                         covariance: noise_transform6's, or Eigen's own eigenvectors() * eigenvalues().cwiseSqrt().asDiagonal()
 *                         for the reference's particles value for value. Zero entries, even an all-zero transform, draw like any
 *                         other: the engine always advances by the calls of 3 n_p accepted attempts. -3: NULL or non-finite
 *                         mean7 / transform36, n_p == 0 or > 0x7fffffff / 16, reset_odom_integ not 0 or 1, engine_state as
 *                         below; nothing is touched then, the resident particles stay.
 * On N devices every rank evaluates the accept decisions of the whole stream (deterministic replicas, no collective) and forms
 * the values of its own shard only. -3: NULL or non-finite sigma6 / mean7 / odom_err4, a negative sigma, engine_state NULL or
 * outside [1, 2^31 - 2]. -5: no resident particles; resample_apply_drawn without a plan. All six sigmas zero is legal: nothing
 * is drawn, engine_state is unchanged and the noise states are the means. */
int mcl3dl_hip_noise_transform6(const double* cov36, float* transform36, float* eigenvalues6 /*or NULL*/);
int mcl3dl_hip_group_init_drawn_multivariate(mcl3dl_hip_group* g, const float* mean7, const float* transform36, size_t n_p,
                                             int reset_odom_integ, uint32_t* engine_state);
uint32_t mcl3dl_hip_rng_seed(uint32_t seed);
float mcl3dl_hip_rng_uniform(uint32_t* state, float a, float b);
int mcl3dl_hip_group_add_noise_drawn(mcl3dl_hip_group* g, const float* sigma6, uint32_t* engine_state);
int mcl3dl_hip_group_init_drawn(mcl3dl_hip_group* g, const float* mean7, const float* sigma6, size_t n_p, uint32_t* engine_state);
int mcl3dl_hip_group_draw_odom_noise(mcl3dl_hip_group* g, const float* odom_err4, uint32_t* engine_state);
int mcl3dl_hip_group_resample_apply_drawn(mcl3dl_hip_group* g, const float* sigma6, uint32_t* engine_state);
/* ---- resampling the resident particles in ONE call: the prefix sums on the device ---------------------------------------------
 * pf_->resample(sigma) (src/mcl_3dl.cpp:809, pf.h:187-225) and pf_->resizeParticle(n) (:875-885, pf.h:399-436) without the
 * weights, pstep or initial_p crossing the bus: one wavefront runs `accum += p.probability_` with the serial loop's bits and
 * writes every prefix, forms pstep = accum / (float)n_out, draws initial_p = uniform_real_distribution<float>(0, pstep)(engine_)
 * from the engine state handed in, and the searches read both from a device record.
 *   float_prefix           out_prefix[i] = fl(out_prefix[i - 1] + term[i]) on its own, for introspection and tests; term == NULL:
 *                          every term is `constant` (resizeParticle's pscan += pstep).
 *   resample_plan_device   begin_device + the caller's uniform draw + plan on one context, weights in device memory. Leaves the
 *                          context where mcl3dl_hip_resample_plan does: resample_apply_device / _apply_slice_device follow.
 *                          mode 0: *engine_state in / out; mode 1: ignored, may be NULL. d_weight needs a float's alignment
 *                          only (16-byte aligned arrays are read four floats at a time).
 *   group_resample_drawn   group_resample_begin(0), rng_uniform(state, 0, pstep), group_resample_plan(0, initial_p),
 *                          group_resample_apply_drawn(sigma6, state) in one call: the same particles, weights 1 / n, odometry
 *                          noise, engine state and residency, bit for bit.
 *   group_resize_resident  group_resample_begin(n_out), _plan(1, .), _apply without noise in one call.
 * *out_route: 0 = no tie among the accumulated probabilities: on a group of one device nothing proportional to the particle
 * count crossed the bus (two fixed-size read-backs: the record, and the duplicate count that sizes the noise draw). 1 = some
 * i > 0 has !(accum[i - 1] < accum[i]) (weight-0 particles, weights below half an ulp of the running sum): libstdc++'s
 * std::sort decides who leads each tie group, so the keys come to the host, are sorted there and the order goes up, as in
 * mcl3dl_hip_resample_begin; the result is the same, only slower. On N devices every rank needs all weights in particle order:
 * one ncclAllGather of the weight shards, or through the host with "collective" 1. Measured on one MI355X the one-call forms
 * are the faster ones up to 65 536 particles without ties and the slower ones at 262 144 and on route 1.
 * -3: NULL d_weight, n or n_out outside its range, bad mode, sigma6 / engine_state as above. -5: no resident particles. */
int mcl3dl_hip_float_prefix(mcl3dl_hip_ctx* ctx, const float* term /*n, host; NULL = constant*/, float constant, size_t n,
                            float* out_prefix /*n, host*/);
int mcl3dl_hip_resample_plan_device(mcl3dl_hip_ctx* ctx, const float* d_weight /*n*/, size_t n, size_t n_out, int mode,
                                    uint32_t* engine_state, float* out_pstep, float* out_initial_p, size_t* out_n_duplicates,
                                    int* out_route);
int mcl3dl_hip_group_resample_drawn(mcl3dl_hip_group* g, const float* sigma6, uint32_t* engine_state, float* out_pstep,
                                    float* out_initial_p, size_t* out_n_duplicates, int* out_route);
int mcl3dl_hip_group_resize_resident(mcl3dl_hip_group* g, size_t n_out, int* out_route);
int mcl3dl_hip_group_measure_landmark(mcl3dl_hip_group* g, const float* measured7, const double* cov36,
                                      float* out_weight /*n_p or NULL*/, float* out_lik /*n_p or NULL*/, float* entropy,
                                      int* restored);
/* ---- occupied bins of the particles: KLD size and modes (NOT the reference's behaviour) ------------------------------------
 * The reference shrinks the particle set by a fixed factor per scan (src/mcl_3dl.cpp:875-885) and publishes one mean. These
 * calls give a caller what it needs to size the set by the posterior instead (KLD-sampling, Fox 2003) and to read the
 * hypotheses themselves: which cells of a pose grid the particles occupy, by how many particles and by how much weight.
 * Nothing calls them unless the caller does. Definitions (mcl_3dl_amd/csrc/particle_bins.h states them once for host and device):
 *   position bin  pcl::VoxelGrid's expression with bin_xyz[a] in place of the leaf: inv = 1.0f / bin in float,
 *                 i_a = (int)(floorf(p_a * inv_a) - (float)min_b_a), min_b / max_b from the min / max over the particles with
 *                 finite positions; the index reported is the absolute one, i_a + min_b_a.
 *   yaw sector    t0, t1 as Quat::getRPY forms them (include/mcl_3dl/quat.h:193-195); no atan2: the first j in 0 ... yaw_bins - 1
 *                 with c_j (double)t1 - s_j (double)t0 >= 0 and c_{j+1} (double)t1 - s_{j+1} (double)t0 < 0 (products and
 *                 difference in double, unfused, the table wrapping around); 0 when no j qualifies (t0 = t1 = 0, a non-finite
 *                 quaternion) and always with yaw_bins = 1. yaw_bins is 1 or 3 ... 64.
 *   key           ((i2 div1 + i1) div0 + i0) yaw_bins + sector, div_a = max_b_a - min_b_a + 1; -3 ("the bins are too small for
 *                 the particles' extent") when div0 div1 div2 yaw_bins > 0xfffffffe or one div_a > 2^31 - 1. A particle with a
 *                 non-finite position sits in no bin and is counted in *out_nonfinite.
 *   per bin       count; mass = the sum of the float weights in fp64; leader = the particle with the largest weight, the lowest
 *                 index on a tie (the strict `<` of pf::max()).
 *   totals        *out_occupied = bins with a particle, *out_occupied_alive = bins with mass > 0.
 *   top K         the top_k (0 ... 16) bins by mass descending, then key ascending: out_top_bin4 = {ix, iy, iz, sector} each,
 *                 out_top_mass, out_top_count, out_top_leader; *out_top_n = min(top_k, occupied) rows are written.
 * Two calls on the same data return the same bits. Any out_* pointer may be NULL. -3: n = 0, a bin edge <= 0, a bad yaw_bins /
 * top_k / row_stride.
 *   _yaw_sector_table  pure host function, no context: out_cs[2 j], out_cs[2 j + 1] = (cos, sin)(2 pi j / yaw_bins), the
 *                 multiples of a quarter turn exact — the very table the device calls use. -3 for a bad yaw_bins.
 *   _kld_bound    pure host function: Fox's bound as AMCL's pf_resample_limit writes it, in double: b = 2 / (9 (k - 1)),
 *                 x = 1 - b + sqrt(b) z, n = ceil((k - 1) / (2 epsilon) x x x); k <= 1 -> 1 (and never less than 1). -3 for
 *                 epsilon outside (0, 1], a non-finite z, a bound that does not fit 2^62. Clamping to the node's
 *                 num_particles_ is the caller's.
 *   _device       n rows of row_stride floats in device memory (7: pose rows, 13: state rows; position at 0..2, quaternion
 *                 xyzw at 3..6) and n weights. Synchronises twice: the extent, then one record with the top rows.
 *   group form    the resident particles, leaders as global particle indices. On more than one rank states and weights are
 *                 brought into particle order on every rank as the resampling plan's weights are, every rank runs the same
 *                 pipeline and the results must agree (-4 otherwise). -5: no resident particles. */
int mcl3dl_hip_yaw_sector_table(int yaw_bins, double* out_cs /*2 * yaw_bins*/);
int mcl3dl_hip_kld_bound(size_t k, double epsilon, double z, size_t* out_n);
int mcl3dl_hip_particle_bins_device(mcl3dl_hip_ctx* ctx, const float* d_rows, size_t row_stride, const float* d_weight, size_t n,
                                    const float* bin_xyz, int yaw_bins, int top_k, size_t* out_occupied,
                                    size_t* out_occupied_alive, size_t* out_nonfinite, int32_t* out_top_bin4 /*4 * top_k*/,
                                    double* out_top_mass, uint32_t* out_top_count, uint32_t* out_top_leader, size_t* out_top_n);
int mcl3dl_hip_group_particle_bins(mcl3dl_hip_group* g, const float* bin_xyz, int yaw_bins, int top_k, size_t* out_occupied,
                                   size_t* out_occupied_alive, size_t* out_nonfinite, int32_t* out_top_bin4 /*4 * top_k*/,
                                   double* out_top_mass, uint32_t* out_top_count, uint32_t* out_top_leader, size_t* out_top_n);
/* ---- global localisation: the particle set seeded from the map, on the devices ---------------------------------------------
 * The reference's `global_localization` service (cbGlobalLocalization, src/mcl_3dl.cpp:1039-1099), step by step:
 *   1. pcl::VoxelGrid(leaf = (float)grid) over pc_map_: the BASE map only, a map update overlay is ignored;
 *   2. a KdTreeFLANN over the centroids with the map's dist_weight; centroid p is dropped when
 *      radiusSearch(p2, grid, ..., 1) finds anything, p2 = p with p2.z = (float)((double)p.z + (0.01 + grid)): some centroid c
 *      (p itself included) has d2(c, p2) < (float)(grid * grid) in the rescaled metric, flann::L2_Simple float arithmetic;
 *   3. remove_if / erase: the survivors ("standable" points) keep their VoxelGrid order;
 *   4. resizeParticle(points * div_yaw); particle i = point i / div_yaw with rotation i % div_yaw,
 *      (Quat(Vec3(0, 0, 2 pi cnt / div_yaw)) * imu_quat).normalized(), probability (float)(1.0 / (float)points) — one over the
 *      number of POINTS —, both odom_err_integ_* and the odometry noise zero.
 * Points, rotations and weights are the reference's bit for bit: the div_yaw rotations are formed on the host (the host's
 * cosf / sinf, as the reference forms them) and handed to the seeding kernel as a table.
 *   _rotations    pure host function, no context: out_quat4 = div_yaw x {x, y, z, w}; imu_quat4 NULL = identity. -3 for
 *                 div_yaw < 1, a NULL output or a non-finite quaternion.
 *   _points       steps 1-3 on one context. The surviving points stay on the device for _seed_device — until the next map
 *                 call — and are returned when out_xyz != NULL (capacity in points; -3 when too small, *n_points still set).
 *                 *n_centroids = leaves of step 1. The context's map index is neither used nor rebuilt: the centroids are
 *                 searched through a cell grid of their own ("Global localisation"), which is refused with -3 when
 *                 a large dist_weight stretches the centroid cloud over more than 2^28 cells of edge 1.01 grid.
 *   _seed_device  step 4 for particles [first, first + count) of the global order into caller-owned device arrays (any may be
 *                 NULL), each starting at particle `first`: 13-float states, 7-float poses, weights.
 *   group form    the service: every rank runs steps 1-3 on its replica of the map (deterministic, no collective) and seeds its
 *                 own shard (mcl3dl_hip_group_shard). Afterwards *n_particles = *n_points * div_yaw particles are RESIDENT,
 *                 exactly as after mcl3dl_hip_group_upload_state with the same states and weights (no odometry noise, no
 *                 resampling in progress). With one device and "direct_single" 1 no thread and no RCCL is touched.
 * Errors, all of which leave previously resident particles untouched: -5 no map; -3 grid <= 0, div_yaw < 1, non-finite
 * imu_quat4; -5 "no standable point" when nothing survives step 2 (every centroid finds ITSELF when
 * dist_weight_z * (0.01 + grid) < grid; the reference would resizeParticle(0)); -3 when the particles needed exceed
 * max_particles (0 = no cap) or what upload_state accepts — the message names the count, *n_points / *n_particles are set. */
int mcl3dl_hip_global_localization_rotations(int div_yaw, const float* imu_quat4 /*NULL = identity*/,
                                             float* out_quat4 /*div_yaw*4*/);
int mcl3dl_hip_global_localization_points(mcl3dl_hip_ctx* ctx, double grid, float* out_xyz /*capacity*3 or NULL*/,
                                          size_t capacity, size_t* n_points, size_t* n_centroids);
int mcl3dl_hip_global_localization_seed_device(mcl3dl_hip_ctx* ctx, int div_yaw, const float* imu_quat4, size_t first,
                                               size_t count, float* d_state13, float* d_pose7, float* d_weight);
int mcl3dl_hip_group_global_localization(mcl3dl_hip_group* g, double grid, int div_yaw, const float* imu_quat4,
                                         size_t max_particles /*0 = no cap*/, size_t* n_points, size_t* n_particles);
/* ---- normal-weighted scan sampling: point normals and sampling weights on the device -----------------------------------------
 * The reference's second sampler, PointCloudSamplerWithNormal (point_cloud_sampler_with_normal.h; the node's
 * use_random_sampler_with_normal), up to its first random draw:
 *   _direction       pure host function, no context: setParticleStatistics (:75-89), the max_weight ladder (:110-127) and
 *                    fpc_local (:128-129). pos_cov(i, j) = |cov36[6 i + j]| for i, j < 3 as doubles (lower triangle read, as Eigen's
 *                    SelfAdjointEigenSolver reads it), symmetric eigen-decomposition in double, eigenvalues ascending,
 *                    ratio = sqrt(l2 / l1), the three-way branch as written there (a NaN ratio fails both comparisons),
 *                    fpc_global = the eigenvector of l2 narrowed to float (its sign is arbitrary, the weights use |.|),
 *                    fpc_local = rot.inv() * fpc_global in the reference's float Quat arithmetic. -3 for a NULL mean7 / cov36 /
 *                    out_fpc_local3 / out_max_weight or a non-finite input.
 *   _normal_weights  :130-158 on a cloud mcl3dl_hip_scan_begin left on the device (which = 0 pc_local_full, 1 / 2 the clipped
 *                    likelihood / beam cloud), in the cloud's order. pcl::NormalEstimation is not pinned by the reference, so
 *                    the normal is defined here: neighbours of point i = every j, i included, with
 *                    d2 = ((dx dx) + dy dy) + dz dz < (float)(r r) in float, plain metric (mcl3dl_hip_radius_search's expression; a
 *                    non-finite point is nobody's neighbour); fewer than 3: normal NaN, weight 1; else moments in double about
 *                    the query, normal = unit eigenvector of the smallest eigenvalue of the covariance (fp64 cyclic Jacobi),
 *                    c = min(1, |n . fpc_local|), weight = 1 + (max_weight - 1) ((pi/2 - acos c) / (pi/2)), all in double.
 *                    out_cumulative[i] = weight[i] + out_cumulative[i - 1]: the reference's sequential double recurrence, run on
 *                    the host over the downloaded weights. out_normal_xyz: the normals narrowed to float, sign arbitrary.
 *                    capacity in points. *n = points of the cloud, *n_without_normal = points with fewer than 3 neighbours.
 * The caller runs the draw (:159-177: uniform_real_distribution over [0, out_cumulative[n - 1]), lower_bound, unordered_set) with
 * its own std::default_random_engine and hands the indices to mcl3dl_hip_scan_finish — or leaves all of it on the device with
 * mcl3dl_hip_scan_finish_drawn_normal below; when the cloud has no more points than
 * asked for (:104-108) no weights are needed at all. The prepared clouds, the installed scans, the map's indices and a current
 * global-localisation point set are left as they are.
 * Errors of _normal_weights: -5 without a preceding mcl3dl_hip_scan_begin; -3 for which outside 0..2, a normal_search_range
 * that is not positive and finite, non-finite fpc_local3 / max_weight, capacity < *n with an output array given (*n is still
 * set), or a cloud whose cell grid (edge 1.01 normal_search_range) would need more than 2^28 cells — the message names the count.
 * An empty cloud returns 0 with nothing written. */
int mcl3dl_hip_sampler_normal_direction(const float* mean7 /*px,py,pz,qx,qy,qz,qw*/, const float* cov36 /*row-major 6x6*/,
                                        double perform_weighting_ratio, double max_weight_ratio, double max_weight,
                                        float* out_fpc_local3, double* out_max_weight, double* out_eigen_value_ratio /*or NULL*/);
int mcl3dl_hip_scan_normal_weights(mcl3dl_hip_ctx* ctx, int which, double normal_search_range, const float* fpc_local3,
                                   double max_weight, double* out_cumulative /*n or NULL*/, float* out_normal_xyz /*n*3 or NULL*/,
                                   size_t capacity, size_t* n, size_t* n_without_normal /*or NULL*/);
/* ---- prepared scans on a device group, the uniform sampler drawn on the devices -----------------------------
 * Replaces: PointCloudUniformSampler::sample (point_cloud_uniform_sampler.h:58-75) for both measurement models, and the scan
 * take-over of a group's update. measure() (src/mcl_3dl.cpp:377-383) walks lidar_measurements_, a std::map<std::string, ...>:
 * "beam" filters — and draws — BEFORE "likelihood", both through the one sampler_ and its one std::default_random_engine. One
 * scan's stream is therefore n_b draws of std::uniform_int_distribution<size_t>(0, n_beam_clipped - 1), then n_s draws over
 * [0, n_lik_clipped); sample() returns an empty cloud WITHOUT drawing when its input is empty (:63-64), and num == 0 draws
 * nothing. libstdc++'s uniform_int_distribution over minstd_rand0 is restated per attempt (mcl_3dl_amd/csrc/rng_index.h): ranges
 * up to 2147483646 values; the up-scaling branch above that is refused. engine_state is in / out as for the drawn noise above and
 * is left untouched by any error.
 *   rng_draw_indices           count draws of uniform_int_distribution<size_t>(0, range - 1) from the engine, on one context;
 *                              out_idx on the host. Introspection and general use.
 *   scan_finish_drawn          mcl3dl_hip_scan_finish with both index arrays drawn on the device: the indices never exist on the
 *                              host, and from the index buffer on the call IS scan_finish (same gather, same ordering, same scan
 *                              state). A model whose clipped cloud is empty or whose count is 0 draws nothing and gets an empty
 *                              scan; *out_n_s / *out_n_b (may be NULL) report what was installed. Up to 65536 draws take one
 *                              launch and no synchronisation beyond the one scan_finish has; more run in rounds per model.
 *   group_scan_begin / _begin_pointcloud2 / _finish / _finish_drawn
 *                              the context forms on every rank, each on its own replica of the cloud (deterministic, no
 *                              collective). The sizes and the engine state of all ranks must agree, else -4. With one device and
 *                              "direct_single" 1 each is the plain call on the context. mcl3dl_hip_scan_download and
 *                              mcl3dl_hip_scan_normal_weights keep working on mcl3dl_hip_group_context(g, 0) behind a
 *                              group_scan_begin: the normal-weighted sampler serves a group through group_scan_finish with
 *                              caller-drawn indices.
 *   group_update_resident_prepared
 *                              mcl3dl_hip_group_update_resident on the scans the group's scan_finish (either form) installed:
 *                              no scan argument, nothing is taken over. The installed scans stay until something installs
 *                              others (a host-scan update replaces them, as before).
 * -3: range 0 or above 2147483646, engine_state NULL or outside [1, 2^31 - 2], n_b > 0 without origins, and what scan_finish
 * refuses. -5: no prepared scan; update_resident_prepared without resident particles, or without installed scans of equal
 * (n_s, n_b, n_o) on every rank — the message names the rank. */
int mcl3dl_hip_rng_draw_indices(mcl3dl_hip_ctx* ctx, uint64_t range, size_t count, uint32_t* engine_state,
                                uint32_t* out_idx /*count*/);
int mcl3dl_hip_scan_finish_drawn(mcl3dl_hip_ctx* ctx, size_t n_s, size_t n_b, const float* origins /*n_o*3*/, size_t n_o,
                                 uint32_t* engine_state, size_t* out_n_s, size_t* out_n_b);
int mcl3dl_hip_group_scan_begin(mcl3dl_hip_group* g, const float* xyz /*n*3*/, const uint32_t* label /*n or NULL*/, size_t n,
                                const float* leaf3, const float* clip_lik4, const float* clip_beam4, size_t* n_full,
                                size_t* n_lik_clipped, size_t* n_beam_clipped);
int mcl3dl_hip_group_scan_begin_pointcloud2(mcl3dl_hip_group* g, const uint8_t* data, size_t n_points, uint32_t point_step,
                                            int off_x, int off_y, int off_z, int off_label, uint32_t label_override,
                                            const float* leaf3, const float* clip_lik4, const float* clip_beam4, size_t* n_full,
                                            size_t* n_lik_clipped, size_t* n_beam_clipped);
int mcl3dl_hip_group_scan_finish(mcl3dl_hip_group* g, const uint32_t* idx_lik /*n_s*/, size_t n_s,
                                 const uint32_t* idx_beam /*n_b*/, size_t n_b, const float* origins /*n_o*3*/, size_t n_o);
int mcl3dl_hip_group_scan_finish_drawn(mcl3dl_hip_group* g, size_t n_s, size_t n_b, const float* origins /*n_o*3*/, size_t n_o,
                                       uint32_t* engine_state, size_t* out_n_s, size_t* out_n_b);
int mcl3dl_hip_group_update_resident_prepared(mcl3dl_hip_group* g, const float* extra /*n_p or NULL*/, float* out_weight,
                                              float* out_lik, float* out_match_ratio, float* out_beam, float* entropy,
                                              float* match_ratio_min, float* match_ratio_max, int* restored);
/* ---- clouds accumulated on the device: accum_cloud > 1 and several sensors without a host cloud -----------
 * Replaces: accumClear and accumCloud (src/mcl_3dl.cpp:267-302) and the head of measure() (:312-336) in front of what
 * mcl3dl_hip_scan_begin replaces. The accumulation logic (src/cloud_accum.cpp), the tf lookups and the per-cloud origins
 * (:343-359) stay the caller's.
 *   scan_accum_clear           accumClear: the accumulation is empty again, the next push gets index 0.
 *   scan_accum_push            accumCloud for one message: every point is transformed by affine12 — the rows of the 3x4 [R | t],
 *                              odom <- sensor —, labelled with the number of clouds pushed since the last clear and appended.
 *                              *out_cloud_index (may be NULL) = that label, *out_total_points (may be NULL) = the points held
 *                              afterwards. Returns once `xyz` may be reused; the work is enqueued on the context's stream.
 *   scan_accum_push_pointcloud2  the same from the wire format (layout rules: mcl3dl_hip_pointcloud2_layout_ok above). The
 *                              message's own label field is not read — accumCloud overwrites it —, hence no off_label.
 *   scan_accum_size            clouds pushed since the last clear, points held.
 *   scan_accum_download        the accumulation as held: odom frame, push order, label = cloud index (xyz NULL: only *n).
 *   scan_begin_accumulated     transforms the accumulation by affine12 (base_link <- odom at the last stamp) into the scan path's
 *                              raw cloud, then VoxelGrid + both clips exactly as mcl3dl_hip_scan_begin on that cloud; whatever
 *                              follows a scan_begin follows it unchanged. The accumulation is NOT consumed: a second call gives
 *                              the same bits, a later push continues with the next index, clearing is the caller's accumClear.
 *                              No point travels host to device in this call.
 * The arithmetic of both transforms, per output row r, in float32, every product and sum rounded on its own (no fused
 * multiply-add):  out[r] = ((m[r][0] x + m[r][1] y) + m[r][2] z) + m[r][3].  The two transforms are not composed: between them
 * the points are floats in the odom frame, as pc_local_accum_ holds them. affine12 == NULL copies the coordinates' bits.
 * Non-finite coordinates get no special treatment (VoxelGrid drops them). The reference has this arithmetic from
 * tf2_sensor_msgs and PCL over an Eigen it neither vendors nor pins: parity is against this statement.
 * The caller builds the matrix with its own Eigen:
 *   Eigen::Matrix<float, 3, 4, Eigen::RowMajor> m = (Eigen::Translation3f(..) * Eigen::Quaternionf(w, x, y, z)).matrix().topRows<3>();
 * -3 (every argument is checked before anything is modified; a refused push consumes no index and leaves the accumulation as it
 * was): an empty cloud ("Given PointCloud2 is empty", point_conversion.h:54-58, where accumCloud returns false), a NULL array,
 * a field offset that does not fit point_step, a non-finite entry of affine12, more than 2^31 - 1 points in total. -5:
 * scan_begin_accumulated with nothing pushed ("MCL measure function is called without available pointcloud", :312-316); a
 * scan prepared earlier stays usable.
 * group_*: the context forms on every rank, each on its own replica (mcl3dl_hip_group_scan_begin's rules: the ranks must agree,
 * else -4). The accumulation of rank r is read with mcl3dl_hip_scan_accum_download on mcl3dl_hip_group_context(g, r). */
int mcl3dl_hip_scan_accum_clear(mcl3dl_hip_ctx* ctx);
int mcl3dl_hip_scan_accum_push(mcl3dl_hip_ctx* ctx, const float* xyz /*n*3, sensor frame*/, size_t n,
                               const float* affine12 /*or NULL*/, size_t* out_cloud_index, size_t* out_total_points);
int mcl3dl_hip_scan_accum_push_pointcloud2(mcl3dl_hip_ctx* ctx, const uint8_t* data, size_t n_points, uint32_t point_step,
                                           int off_x, int off_y, int off_z, const float* affine12 /*or NULL*/,
                                           size_t* out_cloud_index, size_t* out_total_points);
int mcl3dl_hip_scan_accum_size(mcl3dl_hip_ctx* ctx, size_t* n_clouds, size_t* n_points);
int mcl3dl_hip_scan_accum_download(mcl3dl_hip_ctx* ctx, float* xyz, uint32_t* label, size_t capacity, size_t* n);
int mcl3dl_hip_scan_begin_accumulated(mcl3dl_hip_ctx* ctx, const float* affine12 /*or NULL*/, const float* leaf3,
                                      const float* clip_lik4, const float* clip_beam4, size_t* n_full, size_t* n_lik_clipped,
                                      size_t* n_beam_clipped);
int mcl3dl_hip_group_scan_accum_clear(mcl3dl_hip_group* g);
int mcl3dl_hip_group_scan_accum_push(mcl3dl_hip_group* g, const float* xyz /*n*3*/, size_t n, const float* affine12 /*or NULL*/,
                                     size_t* out_cloud_index, size_t* out_total_points);
int mcl3dl_hip_group_scan_accum_push_pointcloud2(mcl3dl_hip_group* g, const uint8_t* data, size_t n_points, uint32_t point_step,
                                                 int off_x, int off_y, int off_z, const float* affine12 /*or NULL*/,
                                                 size_t* out_cloud_index, size_t* out_total_points);
int mcl3dl_hip_group_scan_accum_size(mcl3dl_hip_group* g, size_t* n_clouds, size_t* n_points);
int mcl3dl_hip_group_scan_begin_accumulated(mcl3dl_hip_group* g, const float* affine12 /*or NULL*/, const float* leaf3,
                                            const float* clip_lik4, const float* clip_beam4, size_t* n_full,
                                            size_t* n_lik_clipped, size_t* n_beam_clipped);
/* ---- the normal-weighted sampler drawn on the device ------------------------------------------------------
 * Replaces: lines :139-177 of PointCloudSamplerWithNormal::sample — the cumulative weights (a sequential double recurrence), the
 * std::uniform_real_distribution<double>(0, total) draws, std::lower_bound, the duplicate rejection through a
 * std::unordered_set<size_t>, and that container's ITERATION order, which is the order of the sampled cloud — pinned to
 * libstdc++ (mcl_3dl_amd/csrc/rng_weighted.h, double_chain.h). An attempt of the loop takes two engine calls; attempts behind the
 * one that completes the set are never made. The device weights are the project's own; from the weights on,
 * every bit is the reference's. engine_state is in / out and is left untouched by any error.
 *   rng_draw_weighted          weights in, the container's iteration order out (out_idx, num ids), on one context. out_cumulative
 *                              (may be NULL) receives the n cumulative weights, *out_draws (may be NULL) the attempts made.
 *                              num == 0 forms only the cumulative array, of ANY doubles (engine_state may be NULL). num > 0
 *                              needs n > num (a cloud of at most num points is copied by the caller), every weight finite and
 *                              >= 1 and a total below 2^50 — the conditions under which the reference's loop provably ends
 *                              (rng_weighted.h) — else -3.
 *   scan_finish_drawn_normal   mcl3dl_hip_scan_finish with both index arrays made by sample() on the device, "beam" before
 *                              "likelihood" on one stream. Per model: an empty clipped cloud or a count of 0 installs an empty
 *                              scan and draws nothing; a clipped cloud of at most the count is installed whole in its own order,
 *                              nothing drawn, no normals computed; otherwise normals -> weights -> cumulative weights -> draws ->
 *                              order. Up to 1109 points per model take one launch for both models' draws and no synchronisation
 *                              beyond the one scan_finish has; more run in rounds per model. From the index buffer on the call
 *                              IS scan_finish, so group_update_resident_prepared works behind the group form unchanged.
 *   group_scan_finish_drawn_normal  the context call on every rank, each on its own replica; -4 when sizes or engine states disagree.
 * -3: what scan_finish_drawn and scan_normal_weights refuse, max_weight < 1, or n_clipped * max_weight >= 2^50. -5: no prepared
 * scan. */
int mcl3dl_hip_rng_draw_weighted(mcl3dl_hip_ctx* ctx, const double* weight /*n*/, size_t n, size_t num, uint32_t* engine_state,
                                 uint32_t* out_idx /*num or NULL*/, double* out_cumulative /*n or NULL*/,
                                 uint64_t* out_draws /*or NULL*/);
int mcl3dl_hip_scan_finish_drawn_normal(mcl3dl_hip_ctx* ctx, size_t n_s, size_t n_b, const float* origins /*n_o*3*/, size_t n_o,
                                        double normal_search_range, const float* fpc_local3, double max_weight,
                                        uint32_t* engine_state, size_t* out_n_s, size_t* out_n_b);
int mcl3dl_hip_group_scan_finish_drawn_normal(mcl3dl_hip_group* g, size_t n_s, size_t n_b, const float* origins /*n_o*3*/,
                                              size_t n_o, double normal_search_range, const float* fpc_local3, double max_weight,
                                              uint32_t* engine_state, size_t* out_n_s, size_t* out_n_b);
/* ---- the sampled covariance on resident particles, std::shuffle on the device -------------------------------
 * Replaces: pf::covariance(1.0, random_sample_ratio) with random_sample_ratio < 1 (pf.h:304-360; src/mcl_3dl.cpp:373 and :706 while
 * there are more particles than num_particles): std::shuffle(iota(p_num), engine_), the first
 * sample_num = min(p_num, (size_t)((float)p_num * ratio)) indices (a FLOAT product, truncated), the sums over those. Pinned to
 * libstdc++ (mcl_3dl_amd/csrc/rng_shuffle.h): a shuffle of n <= 46340 elements takes the library's pair path and is made ON THE
 * HOST by the serial loop (at most 27 000 engine calls; its indices are uploaded); n >= 46341 takes the single path and is made
 * ON THE DEVICE, by every rank of a group for itself (deterministic, no collective). p_num is n: the early `break` of pf.h:316 once
 * the float weight sum passes pass_ratio is not reproduced, as in every covariance here. Sums as in mcl3dl_hip_covariance: float
 * terms, fp64 accumulation in the list's order, mcl3dl_hip_covariance_finish. engine_state is in / out and is left untouched by
 * any error.
 *   rng_shuffle_prefix         the first m entries of std::shuffle(iota(n), engine) and the state behind the WHOLE shuffle;
 *                              n in [1, 2^31 - 2], m <= n; out_idx on the host. (The device path numbers attempts in 32 bits: a
 *                              shuffle that needs 2^32 attempts or more — n near 2^31 — is refused with -3.)
 *   covariance_window_partial_device
 *                              mcl3dl_hip_covariance_partial_device for one shard of a sharded set: d_pose / d_weight hold the
 *                              particles [window_lo, window_lo + n_window), d_subset names particles of the WHOLE set. Entries
 *                              outside the window contribute nothing and keep their place in the list: with one shard the 22 sums
 *                              are those of covariance_partial_device bit for bit. An empty list or window gives 22 zeros.
 *   group_covariance_sampled   the covariance over caller-drawn indices into the resident particles (global indices, any order,
 *                              each < n_resident): every rank reduces the entries of its shard, 22 doubles per rank are added in
 *                              rank order on the host. An empty shard is no error.
 *   group_covariance_drawn     the same with the shuffle made from *engine_state; *out_n_sampled (may be NULL) = sample_num.
 *                              ratio >= 1: no shuffle, no draw, mcl3dl_hip_group_covariance. Prefer _sampled where the caller
 *                              already holds the indices; see DESIGN.md 3.11 for what either route costs.
 * The installed scans, the map's indices, the resampling plan and the odometry noise are left as they are.
 * -3: NULL arrays, an index >= n_resident, an empty list, a NaN or negative ratio, a ratio that samples no particle (the
 * reference divides by zero), engine_state NULL or outside [1, 2^31 - 2]. -5: no resident particles. */
int mcl3dl_hip_rng_shuffle_prefix(mcl3dl_hip_ctx* ctx, size_t n, size_t m, uint32_t* engine_state, uint32_t* out_idx /*m*/);
int mcl3dl_hip_covariance_window_partial_device(mcl3dl_hip_ctx* ctx, const float* d_pose, const float* d_weight,
                                                size_t n_window, const uint32_t* d_subset, size_t n_subset, size_t window_lo,
                                                const float* mean7, double* d_out22);
int mcl3dl_hip_group_covariance_sampled(mcl3dl_hip_group* g, const float* mean7, const uint32_t* subset /*n_subset*/,
                                        size_t n_subset, float* out_cov36);
int mcl3dl_hip_group_covariance_drawn(mcl3dl_hip_group* g, const float* mean7, float random_sample_ratio, uint32_t* engine_state,
                                      size_t* out_n_sampled /*or NULL*/, float* out_cov36);
/* How many updates went through each kind of collective so far. */
int mcl3dl_hip_group_collective_stats(const mcl3dl_hip_group* g, uint64_t* rccl_all_reduces, uint64_t* host_combines);

/* ---- measurement support ------------------------------------------------------------------------------ */
/* Per-kernel hipEvent timing on the launch stream (off by default). */
int mcl3dl_hip_set_kernel_timing(mcl3dl_hip_ctx* ctx, int enable);
int mcl3dl_hip_get_kernel_time(mcl3dl_hip_ctx* ctx, int kernel_id, double* total_ms, uint64_t* launches);
int mcl3dl_hip_reset_kernel_time(mcl3dl_hip_ctx* ctx);
/* Exact workload counts of the last measure (re-runs the kernels in counting mode; not for timed regions):
 * stats[0] = sum over (particle, point) of K = map points in the 27-cell neighbourhood, [1] = evaluations,
 * [2] = DDA voxel steps, [3] = occupied voxels visited, [4] = map points tested, [5] = rays. */
int mcl3dl_hip_workload_stats(mcl3dl_hip_ctx* ctx, const float* d_pose, size_t n_p, double* stats6);
/* Sizes of the device-resident structures (bytes): [0] cell-grid points, [1] cell-grid index, [2] DDA occupancy bitmap,
 * [3] DDA voxel index, [4] DDA points, [5] candidate-voxel brick table, [6] candidate-voxel run delimiters,
 * [7] candidate points (with lik_index 2: [6] = the 64-byte voxel records, [7] = their overflow records). Structures that
 * were never needed are 0. */
int mcl3dl_hip_memory_footprint(mcl3dl_hip_ctx* ctx, uint64_t* bytes8);
/* Options (no reference counterpart). Round 6 pruned the switchboard: what lost its A/B is gone (the two-launch pf::measure tail,
 * the one-launch sorts, the completion word folded into the last kernel, the device-side resampling prefix, the CSR form of the
 * candidate index, sharper pruning of crowded voxels, the replay's A/B knobs, the dense record grid) and the thresholds nobody
 * needs to move are constants (HISTORY.md R6-7). The 39 keys left — 38 and the test hook at the end of this list — are ALL
 * drawn, in combination, by tests/test_gpu_api_fuzz.py. Each is one row of the table in mcl_3dl_amd/csrc/host_options.h (field,
 * value rule, error text, what it makes the engine rebuild); tests/test_abi.py keeps the fuzz's pool and that table in step.
 * Except for "strict_order" and its thresholds — which select HOW the sums are rounded — results are the same bits for every
 * setting. Every key but the hook can be read back with mcl3dl_hip_get_option. A value outside a key's rule is refused with
 * -3 and changes nothing.
 *
 * -- how the sums are added up
 *   "strict_order"      2 (default) = the likelihood terms are added up as the reference adds them — float, sequentially, in the
 *                       order the CALLER's cloud holds its points (likelihood.cpp:120-134) — for every scan of at most
 *                       "strict_exact_max" points (4096: the reference's operating range and far beyond) and for every scan of
 *                       at least "strict_auto_min" points (28 147: from there on three standard deviations of the reference's own
 *                       rounding leave north_star's 1e-5; host_context.h derives it): likelihoods are then the reference's bit for
 *                       bit; so are match ratios and beam scores always, and the normalised weights up to 1024 particles (pf::measure's
 *                       float sum, pf.h:255-260). In between the same float terms are summed in a fixed-order fp64 tree (within
 *                       the reference's rounding of its own float: 5e-6 at 16 384 points). Wherever one work-group owns a
 *                       particle's whole scan (below ~1000 points, or few particles: up to 12 288 points) the exact sum costs no
 *                       memory and no launch — the terms wait in LDS at their original indices and a wavefront runs the
 *                       recurrence 512 terms a pass (float_chain.h); elsewhere it costs an n_s x n_p float buffer and a replay
 *                       launch. When that buffer would take more than half of the free device memory (or "strict_auto_max_bytes",
 *                       or its allocation fails) the launch sums in fp64 instead — an update never fails over it; read-only
 *                       "strict_auto_skipped" counts such launches.
 *                       0 = fp64 tree sums always (fastest; ~1e-6, at worst n_s x 6e-8, from the reference).
 *                       1 = exact always, weights at every particle count too (single GPU); fails loudly when the buffer cannot be had.
 *                       3 = the float recurrence INSIDE the tiled likelihood kernel, at every scan size, over the scan in the
 *                       ENGINE's order (mcl3dl_hip_scan_order): bit-identical to the reference's measure() on the scan permuted
 *                       that way; no term buffer, no replay pass. Suits callers whose scan order means nothing to them (a
 *                       sampled cloud): the drop-in classes with MCL3DL_HIP_ENGINE_ORDER=1.
 *   "strict_exact_max", "strict_auto_min", "strict_auto_max_bytes"   the thresholds above (0 = no cap for the last)
 *   "strict_chunk"      0 (default) = a replay keeps the terms of the whole scan; a point count >= 1024 = scans of at least two such
 *                       chunks are ordered chunk by chunk of the caller's order and replayed with two term buffers (C5: 4.3 GB
 *                       instead of 17 GB, 27.9 instead of 25.6 ms). Same bits. Read-only "scan_chunk_in_use".
 *                       (Mode 3 launches of one DEVICE are serialised across contexts — an event per device —: the hand-off between
 *                       tile work-groups relies on in-order dispatch inside one launch, and two such kernels side by side could starve
 *                       each other's producers. The poll is bounded all the same: ~1 s, then error -2 for that update.)
 *   "scan_presorted"    1 = the caller holds its likelihood scans in the engine's order already (mcl3dl_hip_scan_order_host): no
 *                       ordering launches, the permutation is the identity, and the exact modes follow the caller's own order.
 *   "chain_ppl"         strict_order 3: scan tiles per work-group (0 = four for few particles on long scans, 1, 4). Same bits.
 * -- which kernel runs (same bits)
 *   "lik_index"         2 (default) = candidate-voxel records (map_compiler.h); 0 = 27-cell scan of the cell-sorted map
 *   "lik_tiled", "lik_tiled_min", "lik_group"   tile-major XCD-aware kernel for scans >= lik_tiled_min (1024) points and >= 4 particles;
 *                       particles per work-group 0 (= 16 / 8 / 4 by launch size), 4, 8, 16, 32
 *   "lik_small"         1 = scans of <= 32 points with >= 256 particles share each wavefront between several particles
 *   "lik_coop"          1 = quad-cooperative record fetch + VALU-trimmed evaluation in the tiled kernel
 *   "lik_defer"         1 = overflow rounds queued per wavefront and run densely (packed 64-byte records); 0 = at once; 2 = only on
 *                       maps where enough voxels overflow. Read-only "lik_defer_active"
 *   "lik_tiled_fast"    -1 = the tiled kernel's deferred form runs its pose loop specialised for the common map (records, overflow
 *                       records and brick table below 4 GB, 24-bit table index, packed words, 64-byte records) when the parameters
 *                       allow it (match_dist_flat <= match_dist_min); 0 = never. Same results: a switch for A/B runs and tests.
 *                       Read-only "lik_tiled_fast_active"
 *   "update_small", "update_small_max"   the whole update as ONE launch up to that many particles (512) where the per-particle
 *                       kernels serve the scans; "update_small_conformant" = its arrival tickets as acq_rel RMWs (the memory
 *                       model's form; slower; a mitigation switch, tests/test_gpu_soak.py runs both)
 *   "pf_fused"          1 = pf::measure as ONE work-group up to 1024 particles; 0 = partial + reduce + apply
 *   "overlap_models"    1 = the two models of a large update run side by side: in ONE launch whose work-groups interleave the
 *                       tiled likelihood kernel's and the beam kernel's (fp64-tree sums, >= 64 beam work-groups), else on two
 *                       streams (from 262 144 rays); 0 = behind each other. Same bits either way
 *   "beam_prepare"      1 = launches of >= 32 768 rays take per-(particle, origin) constants from a small kernel
 * -- the likelihood index (same bits)
 *   "cand_voxel_ratio"  voxel edge / match_dist_min; 0 (default) = per map: 0.5, or 0.36 on maps of voxel-filter centroids
 *   "cand_phase"        grid origin phase in voxels, [0, 1) (0.5)
 *   "cand_record_parts" inline candidates per record: 0 (default) / 4 = 64-byte records, 8 = 128-byte records
 *   "cand_packed", "cand_bound"   packed w words / skip bounds in the records when the map allows them
 *   "cand_aniso"        0 = cubes, 1 = boxes that follow the dist_weight (edge of axis a = base edge x min(w_a / w_min,
 *                       "cand_aniso_max" = 8)), 2 (default) = boxes when cubes exceed the budget
 *   "index_budget_bytes"  upper bound of the records: -1 (default) = a quarter of the device's memory, 0 = none; cubes, then boxes,
 *                       then coarser voxels (<= 1.5 r), then a clean error naming the bytes needed. Read-only "index_note" says
 *                       when the index differs from what was asked for; "index_record_bytes", "cand_edge_ratio_x/_y/_z"
 *                       Read-only geometry of the candidate grid in place: "cand_origin_x/_y/_z" (floats), "cand_edge_x/_y/_z",
 *                       "cand_voxels_x/_y/_z", "cand_grow" (the slack of a voxel's grown box: 1e-3 of the shortest edge, more on
 *                       grids longer than ~5 000 voxels; a map that would need more than 1/16 of an edge is refused with -4)
 *   "cand_prune_coop"   1 = the compiler's pruning pass runs 16 lanes per voxel; 0 = one thread per voxel (the form it is checked against)
 *   "grid_build_host"   1 = cell grid and DDA grid built by sequential counting sorts on the host (the form the device builders are
 *                       checked against)
 *   "dda_overlay"       1 = a map update rides on the DDA grid as an overlay instead of forcing a rebuild
 * -- host side
 *   "update_stage", "update_zero_copy"   host-buffer updates: scans / poses / weights taken over by ONE launch that also orders the
 *                       scans; read in place from page-locked memory, results written there by the update's last kernel
 *   "poll_sync", "poll_spin_us"   completion by a polled page-locked word (2 = every synchronisation, 1 = host-buffer updates, 0 =
 *                       hipStreamSynchronize); spin that long (2000 us) before napping between looks
 *   "scan_order_device" scans of at least this many points are ordered on the device (4096; 0 = always on the host)
 *   "batch_slice"       particles per slice of mcl3dl_hip_measure_batch_begin when slice_particles is 0
 *   "timing_mask"       bit k set = kernel group k is timed while kernel timing is on; a value in [0, 2^32)
 *   "test_late_structures"  fault injection for the API-sequence fuzz only */
int mcl3dl_hip_set_option(mcl3dl_hip_ctx* ctx, const char* name, double value);
int mcl3dl_hip_get_option(mcl3dl_hip_ctx* ctx, const char* name, double* value);
/* Candidate-voxel index of the current map: [0] bricks, [1] preliminary candidates, [2] candidates kept,
 * [3] device build time in ms, [4] voxels with at least one candidate, [5] voxels with more candidates than their
 * 64-byte record holds (4), [6] overflow records, [7] voxel edge / match_dist_min in use ([4]..[7]: lik_index 2). */
int mcl3dl_hip_index_stats(mcl3dl_hip_ctx* ctx, double* stats8);

#ifdef __cplusplus
}
#endif
#endif /* MCL3DL_HIP_H */
