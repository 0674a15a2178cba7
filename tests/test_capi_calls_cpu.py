"""CPU tests of mcl_3dl_amd/capi.py's marshalling, without a GPU and without the shared library: Engine and Group objects made
with __new__ call into a stand-in library that logs (symbol, arguments) and returns 0, and the transcript — what reached the
library, what each method returned, what the object keeps alive — is compared with tests/golden/capi_calls.json.

The fixture is the behaviour of the binding BEFORE the context / group calls were given one definition: it was written by
this module's own driver run against that commit's capi.py (regenerate it from a commit whose binding is trusted with
`python tests/test_capi_calls_cpu.py <path to that capi.py> tests/golden/capi_calls.json`), never against the code under test.

Driven: every call in capi.MIRRORED on both classes, and every other method that uses the module's small helpers (_scans,
_f3, _state, _sizes / _ints, _update_result). Where the stand-in has to answer something other than 0 for a method to run at
all it does (RETURNS below: an error text, a resident count). Left out, because they do not run against a stand-in that
writes nothing: none of those methods. Group.context is not driven as a method (it builds an Engine with the real library's
loader); the borrowed Engine it returns is, through Engine._borrowed.
"""
import ctypes as C
import hashlib
import importlib.util
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcl3dl_hip.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "capi_calls.json")
CTX, GRP = "mcl3dl_hip_", "mcl3dl_hip_group_"
# what the stand-in answers where 0 would stop the method: the error texts _check decodes, three resident particles
RETURNS = {CTX + "last_error": b"context text", GRP + "last_error": b"group text", GRP + "resident": 3}


def norm(v):
    """A value that crossed the boundary, or came back from a method, as JSON."""
    if v is None or isinstance(v, str):
        return v
    if isinstance(v, np.ndarray):
        return ["array", str(v.dtype), list(v.shape), bool(v.flags.c_contiguous), hashlib.sha256(v.tobytes()).hexdigest()[:16]]
    if hasattr(v, "_obj"):   # C.byref(x): the pointee's type and the value handed in
        return ["byref", type(v._obj).__name__, norm(v._obj.value)]
    if isinstance(v, C.Array):
        return [type(v).__name__, list(v)]
    if isinstance(v, C._SimpleCData):
        return [type(v).__name__, norm(v.value)]
    if isinstance(v, bytes):
        return ["bytes", v.decode()]
    if isinstance(v, dict):
        return {"dict": [[k, norm(x)] for k, x in v.items()]}
    if isinstance(v, (tuple, list)):
        return [type(v).__name__] + [norm(x) for x in v]
    if isinstance(v, (bool, int, float, np.generic)):
        return [type(v).__name__, v.item() if isinstance(v, np.generic) else v]
    raise TypeError("norm: %r" % (v,))


class Recorder:
    """The stand-in library: every attribute is a function that logs its symbol and arguments and returns 0 (or RETURNS)."""

    def __init__(self):
        self.log, self.owner = [], None

    def __getattr__(self, symbol):
        if symbol.startswith("__"):
            raise AttributeError(symbol)

        def call(*args):
            entry = [symbol] + [norm(a) for a in args]
            if symbol.endswith("measure_batch_begin"):   # the arrays of a batch still open are held across the call
                entry.append(["batch_keep", len(self.owner._batch_keep), norm(self.owner._batch_keep[8])])
            self.log.append(entry)
            return RETURNS.get(symbol, 0)
        return call


def grid(rows, cols, scale=0.25, dtype=np.float32):
    return (np.arange(rows * cols, dtype=np.float64).reshape(rows, cols) * scale - 1.0).astype(dtype)


AFFINE44 = np.vstack([np.hstack([np.eye(3), [[0.5], [-1.5], [2.0]]]), [[0, 0, 0, 1]]])
POSES = grid(3, 7)
STRIDED = grid(5, 6, dtype=np.float64)[:, ::2]   # non-contiguous float64 rows of three
CLOUD2 = grid(4, 4).tobytes()                     # PointCloud2 bytes: x, y, z, label at offsets 0, 4, 8, 12


def shared_steps():
    """(step name, call on an Engine or a Group): every call in capi.MIRRORED, the same inputs for both classes."""
    scan, beam = grid(4, 3), grid(2, 3, 0.5)
    return [
        ("set_map", lambda o: o.set_map(STRIDED)),
        ("set_map label", lambda o: o.set_map(grid(2, 3), label=[7, 9], stamp=5, dist_weight=None)),
        ("set_likelihood_params", lambda o: o.set_likelihood_params(0.3, match_weight=4.0)),
        ("set_beam_params", lambda o: o.set_beam_params(num_points=5, add_penalty_short_only_mode=False)),
        ("set_beam_raycast", lambda o: o.set_beam_raycast(True)),
        ("set_option", lambda o: o.set_option("strict_order", 3)),
        ("upload_poses", lambda o: o.upload_poses(POSES.astype(np.float64))),
        ("measure_batch uploaded", lambda o: o.measure_batch(None, scan)),
        ("measure_batch", lambda o: o.measure_batch(POSES[:2], STRIDED, beam, [1, 0], grid(2, 3, 2.0))),
        ("measure_batch_begin", lambda o: o.measure_batch_begin(POSES, scan, beam, slice_particles=2)),
        ("measure_batch_begin out", lambda o: o.measure_batch_begin(
            None, scan, out=tuple(np.full(3, k, np.float32) for k in (1, 2, 3)))),
        ("measure_batch_wait", lambda o: o.measure_batch_wait(2.0)),
        ("measure_batch_end", lambda o: o.measure_batch_end()),
        ("measure_update", lambda o: o.measure_update(POSES, [0.25, 0.5, 0.25], scan)),
        ("measure_update extra", lambda o: o.measure_update(POSES, np.float64([0.2, 0.3, 0.5]), STRIDED, beam, [0, 1],
                                                             grid(2, 3, 2.0), extra=[1.0, 2.0, 3.0])),
        ("resample_plan", lambda o: o.resample_plan(1, 0.125)),
        ("scan_begin", lambda o: o.scan_begin(STRIDED)),
        ("scan_begin label", lambda o: o.scan_begin(grid(3, 3), label=[1, 2, 3], leaf=(0.1, 0.1, 0.05), clip_lik=None)),
        ("scan_begin_pointcloud2", lambda o: o.scan_begin_pointcloud2(CLOUD2, 4, 16, 0, 4, 8)),
        ("scan_begin_pointcloud2 label", lambda o: o.scan_begin_pointcloud2(CLOUD2, 4, 16, 0, 4, 8, off_label=12,
                                                                             label_override=2, leaf=[0.2, 0.2, 0.2])),
        ("scan_accum_clear", lambda o: o.scan_accum_clear()),
        ("scan_accum_push", lambda o: o.scan_accum_push(STRIDED)),
        ("scan_accum_push affine", lambda o: o.scan_accum_push(grid(2, 3), affine=AFFINE44)),
        ("scan_accum_push_pointcloud2", lambda o: o.scan_accum_push_pointcloud2(CLOUD2, 4, 16, 0, 4, 8, affine=AFFINE44[:3])),
        ("scan_accum_size", lambda o: o.scan_accum_size()),
        ("scan_begin_accumulated", lambda o: o.scan_begin_accumulated()),
        ("scan_begin_accumulated affine", lambda o: o.scan_begin_accumulated(AFFINE44.reshape(-1)[:12], leaf=(0.1, 0.1, 0.1),
                                                                              clip_beam=(1, 2, 3, 4))),
        ("scan_finish", lambda o: o.scan_finish([2, 0, 1])),
        ("scan_finish beam", lambda o: o.scan_finish(None, np.int64([1, 1]), origins=grid(2, 3))),
        ("scan_finish_drawn", lambda o: o.scan_finish_drawn(4, 2, None, 17)),
        ("scan_finish_drawn origins", lambda o: o.scan_finish_drawn(4.0, 2, STRIDED[:2], np.uint32(18))),
        ("scan_finish_drawn_normal", lambda o: o.scan_finish_drawn_normal(4, 2, None, 0.5, [[0, 0, 1]], 5, 19)),
        ("scan_finish_drawn_normal bad", lambda o: o.scan_finish_drawn_normal(4, 2, None, 0.5, [0, 1], 5, 19)),
        ("_check", lambda o: o._check(-7)),
        ("close", lambda o: (o.close(), o.h, o.close())),
    ]


def group_steps():
    cov = np.diag(np.arange(1.0, 7.0))
    return [
        ("update_resident", lambda g: g.update_resident(grid(4, 3))),
        ("update_resident extra, no fetch", lambda g: g.update_resident(STRIDED, grid(2, 3), [1, 0], grid(2, 3),
                                                                        extra=[1, 2, 3], fetch=False)),
        ("update_resident_prepared", lambda g: g.update_resident_prepared()),
        ("update_resident_prepared extra, no fetch", lambda g: g.update_resident_prepared(extra=[1, 2, 3], fetch=False)),
        ("covariance_drawn", lambda g: g.covariance_drawn(POSES[0], 0.5, 21)),
        ("add_noise_drawn", lambda g: g.add_noise_drawn([1, 2, 3, 4, 5, 6], 22)),
        ("init_drawn", lambda g: g.init_drawn(POSES[1], np.ones(6), 3, 23)),
        ("init_drawn_multivariate", lambda g: g.init_drawn_multivariate(POSES[1], cov, 3, 24, reset_odom_integ=True)),
        ("draw_odom_noise", lambda g: g.draw_odom_noise([1, 2, 3, 4], 25)),
        ("resample_apply_drawn", lambda g: g.resample_apply_drawn(np.ones(6), 26)),
        ("resample_drawn", lambda g: (g.resample_drawn(np.ones(6), 27), g._rs_n_out)),
        ("measure_imu", lambda g: g.measure_imu([0, 0, 9.8], 0.1)),
        ("measure_imu no fetch", lambda g: g.measure_imu([0, 0, 9.8], 0.1, fetch=False)),
        ("measure_landmark", lambda g: g.measure_landmark(POSES[2], cov)),
        ("measure_landmark no fetch", lambda g: g.measure_landmark(POSES[2], cov.reshape(-1), fetch=False)),
        ("global_localization", lambda g: g.global_localization(0.5, 4, imu_quat=[0, 0, 0, 1], max_particles=100)),
    ]


def engine_steps(capi):
    return [
        ("pf_measure", lambda e: e.pf_measure([0.5, 0.5], [1, 2])),
        ("pf_measure all", lambda e: e.pf_measure([0.5, 0.5], [1, 2], beam=[3, 4], extra=[5, 6], match_ratio=[7, 8])),
        ("resample_plan no plan", lambda e: e.resample_plan(0, 0.5, want_plan=False)),
        ("resample_plan_device", lambda e: e.resample_plan_device(1234, 5)),
        ("resample_plan_device state", lambda e: e.resample_plan_device(1234, 5, n_out=4, engine_state=28)),
        ("rng_draw_weighted", lambda e: e.rng_draw_weighted([1, 2, 3], 2, 29)),
        ("rng_draw_indices", lambda e: e.rng_draw_indices(10, 3, 30)),
        ("rng_shuffle_prefix", lambda e: e.rng_shuffle_prefix(10, 3, 31)),
        ("set_map_downsampled", lambda e: e.set_map_downsampled(STRIDED, label=[1, 2, 3, 4, 5], leaf=None)),
        ("set_map_pointcloud2", lambda e: e.set_map_pointcloud2(CLOUD2, 4, 16, 0, 4, 8, dist_weight=None)),
        ("map_update", lambda e: e.map_update(None)),
        ("map_update_pointcloud2", lambda e: e.map_update_pointcloud2(CLOUD2, 4, 16, 0, 4, 8, off_label=12)),
        ("upload_scan", lambda e: e.upload_scan(STRIDED, grid(2, 3), None, None)),
        ("borrowed close", lambda e: (lambda b: (b.h, b.device_id, b.close(), b.h))(capi.Engine._borrowed(5, device_id=2))),
    ]


def run_steps(obj, steps):
    out = []
    for name, step in steps:
        obj.lib.log = []
        try:
            result = norm(step(obj))
        except (ValueError, capi_error(obj)) as e:
            result = ["raises", type(e).__name__, str(e)]
        kept = {k: norm(v) for k, v in sorted(vars(obj).items()) if k not in ("lib", "h")}
        out.append({"step": name, "calls": obj.lib.log, "result": result, "keeps": kept})
    return out


def capi_error(obj):
    return sys.modules[type(obj).__module__].EngineError


def drive(capi):
    """The whole transcript of one capi module: the shared steps on both classes, each class's own, the module functions."""
    keep_ptr, keep_load = capi._ptr, capi.load_library
    capi._ptr = lambda a: a   # the log sees the arrays themselves
    try:
        out = {}
        for cls, own in ((capi.Engine, engine_steps(capi)), (capi.Group, group_steps())):
            out[cls.__name__] = []
            for steps in (shared_steps(), own):   # a fresh object each: the shared steps end with close()
                obj = cls.__new__(cls)
                obj.lib, obj.h, obj._rs_n_out = Recorder(), C.c_void_p(1), 3   # (a resample of three slots is pending)
                obj.lib.owner = obj
                capi.load_library = lambda lib=obj.lib: lib
                out[cls.__name__] += run_steps(obj, steps)
                obj.h = obj.lib.owner = None   # nothing left for a __del__ at the collector's whim to log
        lib = Recorder()
        capi.load_library = lambda: lib
        out["module"] = [{"step": "group_shard", "result": norm(capi.group_shard(10, 3, 1))},
                         {"step": "rng_uniform", "result": norm(capi.rng_uniform(32, -1, 1))}, {"calls": lib.log}]
        return json.loads(json.dumps(out))
    finally:
        capi._ptr, capi.load_library = keep_ptr, keep_load


@pytest.fixture(scope="module")
def transcript():
    from mcl_3dl_amd import capi
    return drive(capi)


def test_transcript_is_the_fixtures(transcript):
    want = json.load(open(FIXTURE))
    assert sorted(transcript) == sorted(want)
    for part in want:
        assert len(transcript[part]) == len(want[part])
        for got, exp in zip(transcript[part], want[part]):
            assert got == exp, (part, exp.get("step"))


def shared_logs(transcript, cls):
    names = [name for name, _ in shared_steps()]
    return [e for e in transcript[cls] if e["step"] in names]


def test_every_mirrored_call_is_driven_on_both_classes(transcript):
    from mcl_3dl_amd import capi
    for cls, prefix in (("Engine", CTX), ("Group", GRP)):
        seen = {c[0] for e in shared_logs(transcript, cls) for c in e["calls"]}
        assert seen == {prefix + name for name in capi.MIRRORED}, cls


def test_twins_differ_in_the_symbol_prefix_only(transcript):
    eng, grp = shared_logs(transcript, "Engine"), shared_logs(transcript, "Group")
    assert len(eng) == len(grp) == len(shared_steps())
    for e, g in zip(eng, grp):
        assert e["step"] == g["step"] and e["keeps"] == g["keeps"], e["step"]
        assert len(e["calls"]) == len(g["calls"]), e["step"]
        for ce, cg in zip(e["calls"], g["calls"]):
            assert ce[0].startswith(CTX) and cg[0] == GRP + ce[0][len(CTX):], e["step"]
            assert ce[1:] == cg[1:], e["step"]
        # the results are the same but for the two error texts, which name their handle's kind and read their own last_error
        if e["step"] == "_check":
            assert e["result"] == ["raises", "EngineError", "mcl3dl_hip error -7: context text"]
            assert g["result"] == ["raises", "EngineError", "mcl3dl_hip group error -7: group text"]
        else:
            assert e["result"] == g["result"], e["step"]


def test_group_signatures_are_the_context_entries():
    from mcl_3dl_amd import capi
    assert len(set(capi.MIRRORED)) == len(capi.MIRRORED) == 24
    for name in capi.MIRRORED:
        assert capi.SIGNATURES[GRP + name] is capi.SIGNATURES[CTX + name], name
    source = open(capi.__file__).read()
    for name in capi.MIRRORED:
        assert not re.search(r"\b%s%s\b" % (GRP, name), source), "%s%s is spelled out in capi.py" % (GRP, name)


def declarations():
    """symbol -> (return type, parameter types): the header read as tests/test_abi.py's declared_symbols reads it."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"static inline[^{;]*\{.*?\n\}", "", text, flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(mcl3dl_hip_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        types = [re.sub(r"\s*\b\w+$", "", " ".join(p.split())) if len(p.split()) > 1 else p.strip() for p in params.split(",")]
        out[name] = (" ".join(ret.split()), [t.replace(" *", "*") for t in types])
    return out


def test_header_declares_the_twins_alike():
    """The derived SIGNATURES entry cannot hide a header that drifted: behind the handle the two declarations are the same."""
    from mcl_3dl_amd import capi
    decl = declarations()
    assert sorted(decl) == sorted(capi.SIGNATURES)   # the pattern missed no declaration
    for name in capi.MIRRORED:
        (ret_c, par_c), (ret_g, par_g) = decl[CTX + name], decl[GRP + name]
        assert ret_c == ret_g, name
        assert par_c[0].replace("const ", "") == "mcl3dl_hip_ctx*" and par_g[0].replace("const ", "") == "mcl3dl_hip_group*", name
        assert par_c[0].startswith("const ") == par_g[0].startswith("const "), name
        assert par_c[1:] == par_g[1:], name
        assert len(par_c) == len(capi.SIGNATURES[CTX + name][1]), name


if __name__ == "__main__":
    spec = importlib.util.spec_from_file_location("capi_for_fixture", sys.argv[1])
    module = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = module
    spec.loader.exec_module(module)
    parts = ['"%s": [\n%s\n]' % (part, ",\n".join(json.dumps(step, sort_keys=True) for step in steps))
             for part, steps in sorted(drive(module).items())]
    with open(sys.argv[2], "w") as f:   # one step per line
        f.write("{\n" + ",\n".join(parts) + "\n}\n")
