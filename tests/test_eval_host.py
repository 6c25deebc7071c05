"""The per-stage error table without a GPU: the argument checks of sm_eval_config / sm_upload_truth on a device-less
context, sm_eval_stage_host (the kernels' arithmetic in their order) against exact sums (tests/pyref_stages.py) and
against sm_cal_err, the mask cases, the CPU chain against the oracle's refine(), the stand-alone sanitizer program,
the symbol tables and the facades' plumbing through a recording stand-in for the library."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pyref_stages as PS
from mystereomatching_amd import StereoBatch, StereoMatching, _capi
from mystereomatching_amd import evaluate as E
from mystereomatching_amd import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SHAPES = [(33, 41), (47, 91), (1, 2)]      # odd npix below one block; several blocks and a tail; two pixels
MASK_VALUES = (0, 1, 128, 254, 255)
THRES = (1.0, 2.0)


def _create(p):
    lib = _capi.load()
    ctx = C.c_void_p()
    lib.sm_create(C.byref(ctx), C.byref(p), 0)
    return lib, ctx


def _floats(*v):
    return (C.c_float * len(v))(*v)


# ---- argument checks (host code, before any device call) ---------------------------------------------------------

@pytest.mark.parametrize("args,msg", [
    ((1, 0, 0, _floats(1.0)), b"nthres"), ((1, 0, 5, _floats(1, 2, 3, 4, 5)), b"nthres"),
    ((1, 0, 1, _floats(-1.0)), b"thres[0]"), ((1, 0, 2, _floats(1.0, float("nan"))), b"thres[1]"),
    ((1, 0, 3, _floats(0.0, 1.0, float("inf"))), b"thres[2]"), ((2, 0, 1, _floats(1.0)), b"on must be"),
    ((1, 2, 1, _floats(1.0)), b"keep_maps"), ((1, 0, 1, None), b"thres is null"),
])
def test_eval_config_messages(args, msg):
    lib, ctx = _create(_capi.default_params(15, 32, 32, do_refine=1))
    try:
        assert lib.sm_eval_config(ctx, *args) == _capi.SM_EINVAL
        assert msg in lib.sm_last_error(ctx), lib.sm_last_error(ctx)
        assert lib.sm_eval_config(ctx, 1, 0, 4, _floats(0.0, 0.5, 1.0, 2.0)) == _capi.SM_OK   # +0 is allowed
        assert lib.sm_eval_config(ctx, 0, 0, 0, None) == _capi.SM_OK                           # off: nothing else is read
    finally:
        lib.sm_destroy(ctx)
    assert lib.sm_eval_config(None, 1, 0, 1, _floats(1.0)) == _capi.SM_EINVAL


def test_upload_truth_messages_and_state():
    lib, ctx = _create(_capi.default_params(15, 32, 32, batch_capacity=2))
    gt = np.zeros((3, 32, 32), f32)
    try:
        for n, g, msg in ((1, None, b"gt is null"), (0, gt, b"batch_capacity"), (3, gt, b"batch_capacity"), (-1, gt, b"batch_capacity")):
            assert lib.sm_upload_truth(ctx, n, None if g is None else _capi.ptr(g), None, None, None) == _capi.SM_EINVAL
            assert msg in lib.sm_last_error(ctx), lib.sm_last_error(ctx)
        out = np.zeros((1, 8, 3), _capi.STAGE_ERR_DTYPE)
        assert lib.sm_get_stage_errors(ctx, 1, _capi.ptr(out)) == _capi.SM_ESTATE          # before any run
        assert lib.sm_get_stage_maps(ctx, 1, 0, _capi.ptr(np.zeros((32, 32), np.int16))) == _capi.SM_ESTATE
        assert lib.sm_get_stage_errors(ctx, 0, _capi.ptr(out)) == _capi.SM_EINVAL
        assert lib.sm_get_stage_errors(ctx, 1, None) == _capi.SM_EINVAL
    finally:
        lib.sm_destroy(ctx)
    assert lib.sm_upload_truth(None, 1, _capi.ptr(gt), None, None, None) == _capi.SM_EINVAL
    assert lib.sm_eval_stage_count(None) == 0 and lib.sm_eval_stage_name(None, 0) is None


def test_level_contexts_are_refused_in_source():
    """A pyramid level context needs a device; the call's first statement is what refuses it (the GPU test calls it)."""
    src = open(os.path.join(ROOT, "mystereomatching_amd", "csrc", "sm_eval_host.cpp")).read()
    for fn in ("sm_eval_config", "sm_upload_truth", "sm_get_stage_errors", "sm_get_stage_maps"):
        body = src[src.index("sm_status " + fn + "("):]
        assert re.search(r"\{\s*(//[^\n]*\n\s*)*if \(sm_status r = refuse_level\(c\)\) return r;", body[:600]), fn


@pytest.mark.parametrize("over,want", [
    (dict(), ["wta"]),
    (dict(optimization="so"), ["so"]),
    (dict(optimization=""), ["wta"]),
    (dict(do_refine=1), ["wta", "od", "RV0", "RV1", "pi", "mb"]),
    (dict(do_refine=1, optimization="so", region_vote_nums=3, do_proper_ipol=0), ["so", "od", "RV0", "RV1", "RV2", "mb"]),
    (dict(do_refine=1, do_region_vote=0, do_last_median_blur=0), ["wta", "od", "pi"]),
])
def test_stage_list_before_a_run(over, want):
    """Before any run the list is what the next sm_run would record, from sm_params (the *_config switches need a
    device to come on; the GPU test covers "vmTop", "PKR", "BG" and "da")."""
    lib, ctx = _create(_capi.default_params(15, 32, 32, **over))
    try:
        n = lib.sm_eval_stage_count(ctx)
        assert [lib.sm_eval_stage_name(ctx, i).decode() for i in range(n)] == want
        assert lib.sm_eval_stage_name(ctx, n) is None and lib.sm_eval_stage_name(ctx, -1) is None
    finally:
        lib.sm_destroy(ctx)


# ---- sm_eval_stage_host ------------------------------------------------------------------------------------------

def _case(H, W, seed):
    rng = np.random.default_rng(seed)
    dp = rng.integers(0, 16, (H, W)).astype(np.int16)
    dp[rng.random((H, W)) < 0.15] = rng.choice([-1, -32, -48, -64])
    gt = (rng.random((H, W)) * 15).astype(f32)
    masks = [rng.choice(MASK_VALUES, (H, W)).astype(np.uint8) for _ in range(3)]
    return dp, gt, masks


def _check_against_exact(dp, gt, masks, got):
    want = PS.stage_err(dp, gt, masks, THRES)
    for r in range(3):
        w, g = want[r], got[r]
        assert (int(g["count"]), int(g["invalid"])) == (w["count"], w["invalid"]), r
        assert [int(x) for x in g["bad"]] == w["bad"] + [0, 0], r
        n = w["count"]
        # any order of n - 1 double additions of non-negative terms: (n - 1) 2^-53 relative; twice that is allowed
        assert abs(float(g["sum_sq"]) - w["sum_sq"]) <= n * 2.0 ** -52 * w["sum_sq"], (r, float(g["sum_sq"]), w["sum_sq"])
        if masks[r] is None:
            continue
        for k, t in enumerate(THRES):
            pbm, rms = E.cal_err(dp, gt, masks[r], t)
            assert f32(got.pbm(k)[r]).tobytes() == f32(pbm).tobytes(), (r, k)
            # the reference's float accumulation: at most (n - 1) 2^-24 relative, plus the final roundings
            assert abs(float(got.rms()[r]) - rms) <= rms * (n + 4) * 2.0 ** -24, (r, float(got.rms()[r]), rms)


@pytest.mark.parametrize("H,W", SHAPES)
def test_stage_host_against_exact_sums_and_cal_err(H, W):
    dp, gt, masks = _case(H, W, 100 + H)
    got = E.eval_stage_host(dp, gt, PS.pack((H, W), masks), THRES)
    _check_against_exact(dp, gt, masks, got)
    if H * W > 2:
        assert all(0 < int(got[r]["invalid"]) < int(got[r]["count"]) < H * W for r in range(3))
        assert all(0 < int(got[r]["bad"][1]) < int(got[r]["bad"][0]) for r in range(3))


@pytest.mark.parametrize("H,W", SHAPES)
def test_mask_values_zero_mask_and_null_mask(H, W):
    dp, gt, _ = _case(H, W, 200 + H)
    rng = np.random.default_rng(7)
    graded = rng.choice(MASK_VALUES, (H, W)).astype(np.uint8)
    graded.ravel()[:2] = (255, 254)                      # both kinds are there at every shape
    masks = [graded, np.zeros((H, W), np.uint8), None]
    packed = PS.pack((H, W), masks)
    np.testing.assert_array_equal(packed, E.pack_regions((H, W), *masks))
    np.testing.assert_array_equal(packed, (graded == 255).astype(np.uint8))   # only 255 counts, bit 0 alone
    got = E.eval_stage_host(dp, gt, packed, THRES)
    _check_against_exact(dp, gt, masks, got)
    assert int(got[0]["count"]) == int((graded == 255).sum()) >= 1
    for r in (1, 2):                                      # an all-zero mask and an absent one
        assert int(got[r]["count"]) == 0 and float(got[r]["sum_sq"]) == 0.0
        assert float(got.pbm(0)[r]) == 0.0 and float(got.rms()[r]) == 0.0
    assert E.cal_err(dp, gt, masks[1], 1.0) == (0.0, 0.0)


def test_stage_host_order_is_the_documented_one():
    """The order the header states, restated in numpy for one map of several blocks: thread sums of 8 consecutive
    pixels, the 64-lane tree per wave, the four waves in order, the blocks strided over 64 lanes, the tree again."""
    H, W = 47, 91
    dp, gt, masks = _case(H, W, 5)
    got = E.eval_stage_host(dp, gt, PS.pack((H, W), [masks[0], None, None]), (1.0,))
    dif = np.abs(gt - dp.astype(f32)).astype(f32).astype(np.float64)
    term = np.where(masks[0] == 255, np.where(dp >= 0, dif * dif, 2.0), 0.0).ravel()
    nblk = -(-term.size // 2048)
    term = np.concatenate([term, np.zeros(nblk * 2048 - term.size)]).reshape(nblk, 256, 8)

    def tree(a):                                          # [..., 64] -> [...]
        a = a.copy()
        off = 32
        while off >= 1:
            a[..., :off] = a[..., :off] + a[..., off:2 * off]
            off //= 2
        return a[..., 0]

    thread = np.zeros((nblk, 256))
    for j in range(8):
        thread = thread + term[:, :, j]
    waves = tree(thread.reshape(nblk, 4, 64))
    part = ((waves[:, 0] + waves[:, 1]) + waves[:, 2]) + waves[:, 3]
    lanes = np.zeros(64)
    for b in range(nblk):
        lanes[b % 64] = lanes[b % 64] + part[b]
    assert np.float64(tree(lanes)).tobytes() == np.float64(got[0]["sum_sq"]).tobytes()
    assert nblk == 3


def test_derived_values_and_err_lines():
    raw = np.zeros((2, 3), _capi.STAGE_ERR_DTYPE)
    raw["count"] = [[3, 7, 0], [3, 7, 0]]
    raw["bad"][..., 0] = [[1, 7, 0], [2, 0, 0]]
    raw["sum_sq"] = [[0.75, 14.0, 0.0], [27.0, 0.0, 0.0]]
    t = E.stage_errors_array(raw, ["wta", "mb"])
    assert t.names == ("wta", "mb") and t.pbm().dtype == np.float32 and t.rms().dtype == np.float32
    np.testing.assert_array_equal(t.pbm(), np.array([[f32(1) / f32(3), 1, 0], [f32(2) / f32(3), 0, 0]], f32))
    np.testing.assert_array_equal(t.rms(), np.array([[0.5, np.sqrt(f32(2)), 0], [3, 0, 0]], f32))
    rows = E.err_rows(t, present=(True, True, False))
    assert [(r[0], r[1]) for r in rows] == [("wta", "nonocc"), ("wta", "all"), ("mb", "nonocc"), ("mb", "all")]
    assert E.format_err_lines(rows) == ["wta\tnonocc\tPBM: 0.333333\tRMS: 0.5\tall\tPBM: 1\tRMS: 1.41421\t",
                                        "mb\tnonocc\tPBM: 0.666667\tRMS: 3\tall\tPBM: 0\tRMS: 0\t"]


# ---- the CPU chain -----------------------------------------------------------------------------------------------

def test_chain_ends_in_the_oracles_refine(oracle):
    H, W, D = 40, 70, 16
    pair = S.make_pair(H, W, D, 705)
    cfg = oracle.config(H, W, D - 1, do_refine=1)
    ref = oracle.run_ex(pair, cfg, dumps=("disp_raw", "disp_right"))
    ch = PS.chain(oracle, cfg, ref["disp_raw"], ref["disp_right"], oracle.arms(pair["lbgr"], cfg), pair["lbgr"])
    assert [n for n, _ in ch] == PS.stage_names(cfg) == ["wta", "od", "RV0", "RV1", "pi", "mb"]
    np.testing.assert_array_equal(ch[-1][1], ref["disp"])
    np.testing.assert_array_equal(ch[0][1], ref["disp_raw"])
    assert PS.changed(ch)["od"] > 0 and PS.changed(ch)["pi"] > 0
    plain = oracle.config(H, W, D - 1)
    assert [n for n, _ in PS.chain(oracle, plain, ref["disp_raw"], None, None, None, refine=False)] == ["wta"]


# ---- the stand-alone sanitizer program ---------------------------------------------------------------------------

def test_host_code_under_sanitizers(tmp_path):
    """tests/cpp/eval_host_check.cpp (its own main; sm_eval_core.h's arithmetic and packing) built with
    -fsanitize=address,undefined and run on exactly-sized heap blocks: clean, and bit-equal to the library's
    sm_eval_stage_host."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the stand-alone program")
    exe = str(tmp_path / "eval_host_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "eval_host_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    for (H, W), present in zip(SHAPES, (7, 5, 3)):
        dp, gt, masks = _case(H, W, 300 + H)
        path = tmp_path / f"in_{H}.bin"
        with open(path, "wb") as f:
            for a in [dp, gt] + masks:
                f.write(np.ascontiguousarray(a).tobytes())
        r = subprocess.run([exe, str(H), str(W), str(present), str(path)], capture_output=True)
        assert r.returncode == 0, r.stderr.decode()[-4000:]
        used = [m if present >> i & 1 else None for i, m in enumerate(masks)]
        want = E.eval_stage_host(dp, gt, PS.pack((H, W), used), THRES)
        assert r.stdout == np.asarray(want).tobytes()


# ---- symbol tables, the facades ----------------------------------------------------------------------------------

NEW = ("sm_eval_config", "sm_upload_truth", "sm_eval_stage_count", "sm_eval_stage_name", "sm_get_stage_errors",
       "sm_get_stage_maps", "sm_eval_stage_host")


def test_symbol_tables_and_struct():
    hdr = open(os.path.join(ROOT, "include", "sm_capi.h")).read()
    declared = set(re.findall(r"SM_API\s+[\w\s\*]+?\b(sm_\w+)\s*\(", hdr))
    assert declared == {n for n, _, _ in _capi.SIGNATURES}
    lib = _capi.load()
    for fn in NEW:
        assert fn in declared and hasattr(lib, fn)
    assert C.sizeof(_capi.sm_stage_err) == 32 == np.dtype(_capi.STAGE_ERR_DTYPE).itemsize
    assert _capi.sm_stage_err.sum_sq.offset == 24 == np.dtype(_capi.STAGE_ERR_DTYPE).fields["sum_sq"][1]
    assert _capi.default_params(15, 32, 32).struct_size == C.sizeof(_capi.sm_params) == 216   # no new sm_params field
    assert not any(n.startswith("eval") for n, _ in _capi.sm_params._fields_)
    mk = open(os.path.join(ROOT, "mystereomatching_amd", "csrc", "Makefile")).read()
    assert re.search(r"KERNELS = .*\bsm_eval\b", mk) and re.search(r"HOST = .*\bsm_eval_host\b", mk)


class Recorder:
    """Stands in for the loaded library: every entry point returns SM_OK and is recorded with its arguments."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("sm_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return _capi.SM_OK
        return fn

    def named(self, name):
        return [a for n, a in self.calls if n == name]


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    real = _capi.load()
    r.sm_params_default = real.sm_params_default
    monkeypatch.setattr(_capi, "load", lambda: r)
    return r


def test_stereo_batch_plumbing(rec):
    sb = StereoBatch(15, 32, 40, 2, do_refine=1, eval=dict(on=True, keep_maps=True, thresholds=(1.0, 2.0)))
    (a,) = rec.named("sm_eval_config")
    assert a[1:4] == (1, 1, 2) and list(a[4]) == [1.0, 2.0]
    sb.eval_config(False)
    assert rec.named("sm_eval_config")[-1][1:4] == (0, 0, 1)
    gt = np.zeros((2, 32, 40), f32)
    sb.upload_truth(gt, nonocc=np.zeros((2, 32, 40), np.uint8))
    (u,) = rec.named("sm_upload_truth")
    assert u[1] == 2 and u[3] is not None and u[4] is None and u[5] is None
    with pytest.raises(ValueError):
        sb.upload_truth(np.zeros((2, 32, 41), f32))
    with pytest.raises(ValueError):
        sb.upload_truth(gt, disc=np.zeros((2, 32, 41), np.uint8))
    sb._ctx = None
    rec.calls.clear()
    sb = StereoBatch(15, 32, 40, 2, do_refine=1)          # without the override nothing is called
    assert not rec.named("sm_eval_config") and not rec.named("sm_upload_truth")
    sb._ctx = None
    for fn in ("eval_config", "upload_truth", "stage_names", "stage_errors", "stage_maps"):
        assert callable(getattr(StereoBatch, fn))


def test_stereo_matching_plumbing(rec):
    cls = StereoMatching
    assert cls.Do_stageErrors is False
    z3, z1 = np.zeros((32, 40, 3), np.uint8), np.zeros((32, 40), np.uint8)
    gt = np.zeros((32, 40), f32)
    try:
        for on, dt, calls in ((True, gt, 1), (True, None, 0), (False, gt, 0)):
            rec.calls.clear()
            cls.Do_stageErrors = on
            prm = cls.Parameters(15, 32, 40)
            prm.errorThreshold = 2
            sm = cls(z3, z3, z1, z1, dt, z1, None, z1, param=prm)   # all and disc given, nonocc absent
            assert len(rec.named("sm_eval_config")) == len(rec.named("sm_upload_truth")) == calls
            if calls:
                a = rec.named("sm_eval_config")[0]
                assert a[1:4] == (1, 0, 1) and list(a[4]) == [2.0]
                u = rec.named("sm_upload_truth")[0]
                assert u[1] == 1 and u[3] is None and u[4] is not None and u[5] is not None   # nonocc, all, disc
            else:
                with pytest.raises(_capi.SMError):
                    sm.stageErrors()
            sm._ctx = None
    finally:
        cls.Do_stageErrors = False


def test_cpp_facade_source_and_docs():
    src = open(os.path.join(ROOT, "include", "stereo_matching.hpp")).read()
    for decl in ("inline static bool Do_stageErrors = false;", "std::vector<StageErr> stageErrors()",
                 "sm_eval_config(ctx_, 1, 0, 1, &th)", "sm_get_stage_errors(ctx_, 1, t.data())"):
        assert decl in src, decl
    for name in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "sm_eval_config" in open(os.path.join(ROOT, name)).read(), name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "sm_eval.hip" in design and "sm_eval_stage_host" in design and '"se"' in design


def test_eval_facade_check_compiles(tmp_path):
    """tests/cpp/eval_facade_check.cpp builds against the facade and the library (its rows are compared on the GPU in
    tests/test_gpu_eval.py)."""
    from test_cpp_facade import _compile
    _compile(os.path.join(ROOT, "tests", "cpp", "eval_facade_check.cpp"), str(tmp_path / "eval_facade_check"))



def test_bench_tool_arguments_and_bytes():
    from tools import bench_eval
    a = bench_eval.parse(["--steps", "2", "--warmup", "1", "--rounds", "1", "--batch", "3"])
    assert (a.steps, a.warmup, a.rounds, a.batch, a.rows, a.cols, a.max_disp) == (2, 1, 1, 3, 375, 450, 63)
    assert a.out.endswith(os.path.join("profiles", "eval", "bench_eval_teddy_b16.json"))
    with pytest.raises(SystemExit):
        bench_eval.parse(["--steps", "0"])
    assert bench_eval.eval_bytes(10, False) == 70 and bench_eval.eval_bytes(10, True) == 90
