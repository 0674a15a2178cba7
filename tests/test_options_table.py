"""CPU test of the option table (mcl_3dl_amd/csrc/host_options.h): tests/cpp/options_check.cpp includes that header alone and
checks every row — unique names, a key set to its own default changes nothing, every value the API fuzz draws is accepted and
reads back as stored, values outside a rule (NaN among them) are refused with the field untouched, the test hook needs its
environment variable — and prints each row's default, which must be the DEFAULTS of tests/test_gpu_api_fuzz.py key by key."""
import ast
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def fuzz_pools():
    """DEFAULTS and CHOICES of tests/test_gpu_api_fuzz.py, without importing that module's GPU fixtures."""
    tree = ast.parse(open(os.path.join(HERE, "test_gpu_api_fuzz.py")).read())
    pools = {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", "") in ("DEFAULTS", "CHOICES"):
            pools[node.targets[0].id] = eval(compile(ast.Expression(node.value), "test_gpu_api_fuzz.py", "eval"), {"dict": dict})
    return pools["DEFAULTS"], pools["CHOICES"]


def test_every_row_of_the_option_table(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/bin")
    if not cxx:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "options_check.bin")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mcl_3dl_amd", "csrc"), "-o", exe,
                    os.path.join(HERE, "cpp", "options_check.cpp")], check=True)
    defaults, choices = fuzz_pools()
    args = ["%s=%s" % (k, ",".join(repr(float(v)) for v in vs)) for k, vs in choices.items()]
    env = {k: v for k, v in os.environ.items() if k != "MCL3DL_HIP_TEST_HOOKS"}
    run = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60, env=env)
    print(run.stdout)
    assert run.returncode == 0 and "all checks passed" in run.stdout, run.stdout + run.stderr
    rows = {}
    for line in run.stdout.splitlines()[:-1]:
        name, *values = line.split()
        assert name not in rows, name
        rows[name] = [float(v) for v in values]
    assert set(rows) == set(defaults) | {"test_late_structures"}, sorted(set(rows) ^ set(defaults))
    assert rows.pop("test_late_structures") == [0.0]
    for name, (default, *read_back) in rows.items():
        assert default == float(defaults[name]), (name, default, defaults[name])
        # (every value of the pool survives its conversion: flags are drawn as 0 / 1, counts as whole numbers)
        assert read_back == [float(v) for v in choices[name]], (name, read_back, choices[name])
