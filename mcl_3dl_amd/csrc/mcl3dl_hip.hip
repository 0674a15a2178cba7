// mcl3dl_hip.hip — the one translation unit behind the C ABI of include/mcl3dl_hip.h. Host side in the host_*.h and
// api_*.inl pieces included below (in this order), device code in kernels.h (likelihood / beam / pf / map compiler).
// gfx950 only; there is no CPU fallback anywhere in this library.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <limits>
#include <mutex>
#include <numeric>
#include <string>
#include <vector>

#include <rocprim/rocprim.hpp>  // radix_sort_pairs for whole-map arrays only (host_cloud.h:radix_sort)

#include "kernels.h"
#include "mcl3dl_hip.h"

#pragma clang fp contract(off)

using namespace mcl3dl;

#include "host_options.h"
#include "host_context.h"
#include "host_cloud.h"
#include "host_map_compilers.h"
#include "host_grid_builders.h"
#include "host_measure.h"
#include "host_pf.h"
#include "host_rng.h"
#include "noise_transform.h"
#include "host_weighted.h"
#include "host_shuffle.h"
#include "host_group.h"
#include "host_group_gather.h"

// =================================================================================================================
// C ABI
// =================================================================================================================
extern "C"
{
#include "api_core.inl"
#include "api_reductions.inl"
#include "api_resample.inl"
#include "api_support.inl"
#include "api_cloud.inl"
#include "api_group.inl"
#include "api_group_state.inl"
#include "api_group_motion.inl"
#include "api_global_loc.inl"
#include "api_sampler.inl"
#include "api_rng.inl"
#include "api_shuffle.inl"
#include "api_particle_bins.inl"
}  // extern "C"
