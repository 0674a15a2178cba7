// kernels.h — hand-written gfx950 (CDNA4, wave64) kernels of the LiDAR measurement update.
//
//   likelihood_kernels.h  likelihood-field model: per-particle / small-scan / tile-major (XCD-aware) kernels over the
//                         candidate-voxel index (map_compiler.h) or the cell-sorted map; strict-order sums; radius search
//   likelihood_chain_multi.h  strict_order = 3 for few particles on long scans: several tiles per work-group, a quarter of the hand-offs
//   cell_grid.h           the walk over the cell-sorted map, once: a query's cell, the block of cells within a reach, a row's run,
//                         the nine rows around an interior cell, L2_Simple's distance with the tie rule, cell_grid_nearest (the
//                         definition of the radius search)
//   beam_kernels.h        beam model: one lane per ray, DDA walk through 4x4x4 occupancy bricks, point tests, penalty count; the
//                         model's steps around a caster's walk, once (ray ends, penalty rule and count, HIT / SHORT, score)
//   beam_kd_kernels.h     beam model with the reference's default caster (RaycastUsingKDTree): fixed-step march, exact nearest-
//                         within-radius over the cell-sorted map at every step (cell_grid.h's pieces, loads batched)
//   pf_sums.h             pf::measure's arithmetic, once: the weight product, a particle's terms, the wavefront / block / 64-lane
//                         reductions of {sum w, sum w ln w, max ratio, -min ratio}, the four statistics
//   pf_kernels.h          pf::measure's kernels over pf_sums.h (split, behind the tiled kernel, fused; the float-order weight sum;
//                         normalisation) and the "next" rows (expectation / max / covariance, resampling)
//   motion_kernels.h      between two scans, on resident particles: motion prediction, odometry-error reset, pf::noise, the
//                         scan update's odometry factor, the IMU gravity likelihood (inside pf::measure's partial-sum pass)
//   landmark_kernels.h    on resident particles: the pose-jump bias formed inside the moments pass, the landmark likelihood
//                         (NormalLikelihoodNd<float, 6> over s - measured)
//   update_kernels.h      likelihood + beam + pf::measure (pf_sums.h) in ONE launch for the reference's operating range
//                         (launch-bound sizes)
//   map_compiler.h        device-side compiler of the candidate-voxel index (whole map, or the bricks a map update touches)
//   grid_kernels.h        the cell-sorted exact-NN grid and the DDA occupancy / voxel index, built on the device
//   cloud_kernels.h       scan / map preparation: PointCloud2 decode, VoxelGrid, clip + compaction, sampling gather,
//                         matched / unmatched output (each with the min / max or the count the next step needs fused in)
//   scan_accum.h          the head of measure(): accumCloud (sensor -> odom, label = cloud index, append) and the accumulation's
//                         odom -> base_link pass with VoxelGrid's min / max fused in
//   sort_kernels.h        stable radix sort of the cloud path: keys made in the first pass, points written by the last
//   cloud_keys.h          the sort keys (VoxelGrid leaf index, Morton key, range key)
//   global_loc_kernels.h  global localisation: the blocked-above test over the VoxelGrid centroids of the base map, and the seeding
//                         of points x div_yaw particles into a shard of resident particles
//   rng_stream_kernels.h  the attempt stream the polar, index and shuffle draws share (rng_stream.h: the lane walk and the
//                         placement loop both the device and the CPU emulations compile): one count kernel and one emit kernel
//                         over an attempt policy and a sink, wavefront and work-group ranks
//   rng_kernels.h         the filter's noise from the reference's engine: the polar sink, the noise rows, the odometry noise
//                         (rng_polar.h: the restatement and the polar policy)
//   rng_index_kernels.h   the uniform sampler's index draws from the same engine: the one-work-group form and the index sink
//                         (rng_index.h: the restatement and the index policy)
//   rng_weighted_kernels.h  the normal-weighted sampler's draw: cumulative weights as the serial double recurrence (double_chain.h),
//                         draws, lower_bound, duplicate rejection and the unordered_set's iteration order (rng_weighted.h)
//   rng_shuffle_kernels.h  std::shuffle(iota(n), engine_) of the sampled covariance: the doubt sink, doubtful attempts resolved by one
//                         wavefront, every step's target, one chain walk per entry over the sorted (target, step) pairs
//                         (rng_shuffle.h: the restatement and the doubt policy)
//   resample_prefix_kernels.h  pf::resample / resizeParticle without the host between weights and plan: the accumulated
//                         probabilities and `pscan += pstep` as the serial float recurrence by one wavefront, every prefix
//                         written (float_prefix.h), pstep / initial_p / tie flag in a device record, the search fed from it
//   particle_bins_kernels.h  the occupied bins of a pose grid over the particles (particle_bins.h: the definitions): keys, and a
//                         segmented reduction over the sorted pairs whose cost does not depend on how the particles are spread;
//                         totals and the top K bins by mass
//   stage_kernels.h       head and tail of a host-buffer update as one launch each: scan ordering + pose / weight take-over
//                         from page-locked host memory; lik_finalize + pf::measure with the results written back there
//
// These are gather / traversal kernels (bound by L2/HBM reads and the texture-addresser, not by MFMA):
// there is no dense contraction anywhere on this path, so no matrix-core code.
#pragma once
#include "map_structs.h"
#include "cell_grid.h"
#include "likelihood_kernels.h"
#include "likelihood_chain_multi.h"
#include "beam_kernels.h"
#include "beam_kd_kernels.h"
#include "motion_kernels.h"
#include "pf_kernels.h"
#include "landmark_kernels.h"
#include "update_kernels.h"
#include "cloud_kernels.h"
#include "scan_accum.h"
#include "sort_kernels.h"
#include "stage_kernels.h"
#include "grid_kernels.h"
#include "global_loc_kernels.h"
#include "sampler_kernels.h"
#include "rng_stream_kernels.h"
#include "rng_kernels.h"
#include "rng_index_kernels.h"
#include "rng_weighted_kernels.h"
#include "rng_shuffle_kernels.h"
#include "resample_prefix_kernels.h"
#include "particle_bins_kernels.h"
