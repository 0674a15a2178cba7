"""Writes tests/golden/rng_odom_noise.npz: update_noise_func's stream (src/mcl_3dl.cpp:817-825) — ONE
std::normal_distribution<float>(0, 1) over std::default_random_engine, four values per particle — as the standard library
produces it (tests/cpp/rng_polar_emul.cpp, mode `stream std shared`), with the engine state in front of and behind it."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import rng_ref  # noqa: E402

N_P = 1000
SEED = 4321

if __name__ == "__main__":
    state = rng_ref.minstd_seed(SEED)
    z, behind, _ = rng_ref.stream("std", "shared", state, 4 * N_P)
    np.savez_compressed(os.path.join(HERE, "rng_odom_noise.npz"), z=z.reshape(N_P, 4), state=np.uint32(state),
                        state_behind=np.uint32(behind))
    print("rng_odom_noise.npz: %d particles, engine state %d -> %d" % (N_P, state, behind))
