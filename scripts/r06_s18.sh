#!/bin/bash
# round 6 session 18: the merged launch in front of the caller-order replay where no second stream would be used (below 262 144 rays)
O=gpurun_out/r06x; mkdir -p $O
run() { # name, overlap, bench args
  timeout 900 python bench.py --full $3 --overlap-models $2 2>$O/$1.err | tail -1 > $O/$1.json
  python - "$O/$1.json" "$1" <<'PY'
import json,sys
try:
    d=json.load(open(sys.argv[1])); k=d["kernels_ms_per_step"]
    print("%-24s ms/step %.4f 8d %s lik %.4f beam %.4f pf %.4f err %s" % (sys.argv[2], d["ms_per_step"], d.get("ms_per_step_8d"), k["likelihood"], k["beam"], k["pf"], d["result_check"].get("max_rel_err_vs_cpu")), flush=True)
except Exception as e:
    print(sys.argv[2], "no json", e)
PY
}
Q="--steps 40 --warmup 5 --no-extras --no-cpu-baseline"
for r in 1 2; do
for shape in "4096 2048 48" "4096 4096 48" "2048 4096 96" "8192 1024 16"; do
  set -- $shape
  run p$1x$2+$3_serial_$r 0 "--workload C3 --particles $1 --scan-points $2 --beam-points $3 $Q"
  run p$1x$2+$3_merged_$r 1 "--workload C3 --particles $1 --scan-points $2 --beam-points $3 $Q"
done
done
timeout 1500 python -m pytest tests/test_gpu_launch_paths.py tests/test_gpu_pf_fused.py tests/test_gpu_fuzz.py tests/test_gpu_parity.py tests/test_gpu_api_fuzz.py -m gpu -q 2>&1 | grep -vE "RCCL|HIP version|ROCm version|Hostname|Librccl" | tail -4
