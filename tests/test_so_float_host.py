"""The scan-line optimisers on signed and NaN volumes (sm_create_ex, so_float_minima) without a GPU.

sm_create_ex's argument checks, the refusals that a default sm_create keeps and so_float_minima = 1 lifts, refine()'s
volume-reading stages after "so" (refused with keep_final_volume = 0, accepted with 1), the symbol tables, the facades'
choice of entry point and of keep_final_volume, the restatement (tests/pyref_so_float.py) pinned to the C oracle's
smo_so on the crafted volumes (tests/so_float_cases.py), and the conditions that keep the GPU comparisons on those
volumes from passing vacuously."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pyref_so as P
import pyref_so_float as PF
import so_float_cases as SC
from mystereomatching_amd import StereoBatch, StereoMatching, _capi
from test_da_host import Recorder
from test_so_variants_host import oracle_so, volumes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEF = _capi.SO_PN_DEFAULT
# H, W, D of the crafted volumes for so / so_R2L (so_T2D takes H and W exchanged): every sizeable shape of
# tests/test_gpu_so_float.py's kernel-path list, and the end-to-end / refine / +inf shapes
CRAFTED = [(31, 57, 16), (17, 150, 128), (13, 300, 256), (13, 40, 600), (26, 71, 32), (21, 70, 20), (40, 66, 24)]


def _create_ex(p, opts, dev=0):
    lib = _capi.load()
    ctx = C.c_void_p()
    st = lib.sm_create_ex(C.byref(ctx), C.byref(p), None if opts is None else C.byref(opts), dev)
    return lib, ctx, st


def _create(p):
    lib = _capi.load()
    ctx = C.c_void_p()
    return lib, ctx, lib.sm_create(C.byref(ctx), C.byref(p), 0)


def so_params(**kw):
    kw.setdefault("optimization", "so")
    rows = kw.pop("rows", 32)
    return _capi.default_params(15, rows, 32, **kw)


# what a default sm_create refuses with "so", and its text
REFUSED = [
    (dict(aggregation="GF"), b"aggregation GF (costs may be negative) supports optimization sgm or WTA"),
    (dict(aggregation="GF", gf_mode=1), b"aggregation GF (costs may be negative) supports optimization sgm or WTA"),
    (dict(aggregation="GFNL"), b"aggregation GFNL (costs may be negative) supports optimization sgm or WTA"),
    (dict(aggregation="BF", cost_method="grad"), b"aggregation BF with optimization so is not supported for cost_method grad"),
    (dict(aggregation="BF", cost_method="adGrad"), b"aggregation BF with optimization so is not supported for cost_method adGrad"),
    (dict(aggregation="BF", cost_method="ADCensusGrad"), b"not supported for cost_method ADCensusGrad"),
    (dict(aggregation="BF", cost_method="AD", ad_trunc_ad=1e-30), b"needs ad_trunc_ad a multiple of 2^-25 and <= 1024"),
    (dict(aggregation="BF", cost_method="SD", ad_trunc_ad=2000.0), b"needs ad_trunc_ad a multiple of 2^-25 and <= 1024"),
]


# ---- sm_create_ex ---------------------------------------------------------------------------------------------

def test_opts_default_and_size():
    lib = _capi.load()
    o = _capi.sm_create_opts(struct_size=77, so_float_minima=5)
    lib.sm_create_opts_default(C.byref(o))
    assert (o.struct_size, o.so_float_minima) == (8, 0) and C.sizeof(_capi.sm_create_opts) == 8
    lib.sm_create_opts_default(None)   # tolerated, like sm_params_default
    p = _capi.create_opts(so_float_minima=True)
    assert (p.struct_size, p.so_float_minima) == (8, 1)


@pytest.mark.parametrize("size,fm,msg", [(0, 0, b"sm_create_opts.struct_size"), (12, 1, b"sm_create_opts.struct_size"),
                                         (8, 2, b"so_float_minima"), (8, -1, b"so_float_minima")])
def test_create_ex_argument_checks(size, fm, msg):
    o = _capi.sm_create_opts(struct_size=size, so_float_minima=fm)
    lib, ctx, st = _create_ex(so_params(), o)
    try:
        assert st == _capi.SM_EINVAL and msg in lib.sm_last_error(ctx), lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)
    # before sm_params: a struct that sm_create would refuse for its own size still names the option
    p = so_params()
    p.struct_size = 4
    lib, ctx, st = _create_ex(p, o)
    try:
        assert st == _capi.SM_EINVAL and msg in lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)
    # ... and without a device: an impossible device index changes nothing
    lib, ctx, st = _create_ex(so_params(), o, dev=10 ** 6)
    try:
        assert st == _capi.SM_EINVAL and msg in lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)


def test_create_ex_null_arguments():
    lib = _capi.load()
    assert lib.sm_create_ex(None, C.byref(so_params()), None, 0) == _capi.SM_EINVAL
    ctx = C.c_void_p()
    assert lib.sm_create_ex(C.byref(ctx), None, None, 0) == _capi.SM_EINVAL


@pytest.mark.parametrize("kw,text", REFUSED)
def test_default_contexts_keep_the_refusals(kw, text):
    """sm_create, sm_create_ex with NULL and sm_create_ex with the default options: the same refusal, the same text."""
    for make in (lambda p: _create(p), lambda p: _create_ex(p, None), lambda p: _create_ex(p, _capi.create_opts())):
        lib, ctx, st = make(so_params(**kw))
        try:
            assert st == _capi.SM_EINVAL and text in lib.sm_last_error(ctx), lib.sm_last_error(ctx)
        finally:
            lib.sm_destroy(ctx)


@pytest.mark.parametrize("kw,text", REFUSED)
def test_float_minima_lift_them(kw, text):
    """Validation passes; without a device sm_create_ex then fails for want of one (never SM_EINVAL)."""
    lib, ctx, st = _create_ex(so_params(**kw), _capi.create_opts(so_float_minima=True))
    try:
        assert st != _capi.SM_EINVAL, lib.sm_last_error(ctx)
        assert st == _capi.SM_OK or b"supports optimization" not in lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)


def test_float_minima_change_no_other_check():
    fm = _capi.create_opts(so_float_minima=True)
    for kw, text in ((dict(aggregation="GF", gf_eps=0.0), b"gf_eps"), (dict(aggregation="GF", rows=8), b"needs rows, cols >= 9"),
                     (dict(aggregation="GFNL", nl_sigma=0.0), b"nl_sigma"), (dict(aggregation="BF", rows=6), b"aggregation BF needs rows"),
                     (dict(aggregation=4), b"unknown aggregation"), (dict(num_disparities=0), b"num_disparities")):
        # (on a default context the check is reached with "sgm"; with "so" the refusal of the aggregation precedes some)
        for opts, opt in ((None, "sgm"), (fm, "sgm"), (fm, "so")):
            lib, ctx, st = _create_ex(so_params(optimization=opt, **kw), opts)
            try:
                assert st == _capi.SM_EINVAL and text in lib.sm_last_error(ctx), (kw, lib.sm_last_error(ctx))
            finally:
                lib.sm_destroy(ctx)


@pytest.mark.parametrize("kw", [dict(optimization="sgm"), dict(optimization=""), dict(optimization="sgm", aggregation="GF"),
                                dict(aggregation="CBCA"), dict(aggregation="NL"), dict(aggregation="FIF"), dict(aggregation="AWS"),
                                dict(aggregation="BF"), dict(aggregation="none")])
def test_float_minima_are_accepted_where_nothing_needs_them(kw):
    lib, ctx, st = _create_ex(so_params(**kw), _capi.create_opts(so_float_minima=True))
    try:
        assert st != _capi.SM_EINVAL, lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)


def test_pyramid_levels_are_validated_under_the_owners_option():
    """sm_pyramid_config checks every level as sm_create would: under so_float_minima the levels pass as level 0 did."""
    p = _capi.default_params(31, 64, 64, optimization="so", aggregation="GF")
    lib, ctx, st = _create_ex(p, _capi.create_opts(so_float_minima=True))
    try:
        assert st != _capi.SM_EINVAL
        if st != _capi.SM_OK:   # (a live context would go on to create the levels)
            assert lib.sm_pyramid_config(ctx, 2) == _capi.SM_OK, lib.sm_last_error(ctx)
    finally:
        lib.sm_destroy(ctx)


# ---- refine()'s volume-reading stages after "so" --------------------------------------------------------------

@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("fm", [False, True])
def test_volume_stages_follow_keep_final_volume(variant, fm):
    for keep in (0, 1):
        lib, ctx, st = _create_ex(so_params(do_refine=1, keep_final_volume=keep), _capi.create_opts(so_float_minima=fm))
        try:
            assert st != _capi.SM_EINVAL
            assert lib.sm_so_config(ctx, variant, DEF, DEF) == _capi.SM_OK
            calls = ((lambda: lib.sm_refine_ext_config(ctx, 1, 0.1, -64, 0, 1000, 0, 0), b"do_pkr: not with optimization so"),
                     (lambda: lib.sm_refine_ext_config(ctx, 0, 0.1, -64, 0, 1000, 1, 0), b"do_subpixel: not with optimization so"),
                     (lambda: lib.sm_refine_da_config(ctx, 1, 20, 60, 84, 87), b"sm_refine_da_config: not with optimization so"))
            for call, text in calls:
                if keep:
                    assert call() == _capi.SM_OK, lib.sm_last_error(ctx)
                else:
                    assert call() == _capi.SM_EINVAL and text in lib.sm_last_error(ctx), lib.sm_last_error(ctx)
                    assert b"the reference's so rewrites vm[0] in place" in lib.sm_last_error(ctx)
            # the other argument checks still come first or after, unchanged
            assert lib.sm_refine_ext_config(ctx, 1, float("nan"), -64, 0, 1000, 0, 0) == _capi.SM_EINVAL
            assert b"pkr_ratio" in lib.sm_last_error(ctx)
            assert lib.sm_refine_ext_config(ctx, 0, 0.1, -64, 1, 1000, 0, 0) == _capi.SM_OK   # BGIpol reads no volume
        finally:
            lib.sm_destroy(ctx)


# ---- the symbol tables ---------------------------------------------------------------------------------------

def test_symbol_tables():
    hdr = open(os.path.join(ROOT, "include", "sm_capi.h")).read()
    declared = set(re.findall(r"SM_API\s+[\w\s\*]+?\b(sm_\w+)\s*\(", hdr))
    names = [n for n, _, _ in _capi.SIGNATURES]
    assert declared == set(names) and len(names) == len(set(names))
    sig = {n: (r, a) for n, r, a in _capi.SIGNATURES}
    lib = _capi.load()
    for n in ("sm_create_ex", "sm_create_opts_default"):
        assert n in declared and hasattr(lib, n)
    assert sig["sm_create_ex"] == (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(_capi.sm_params), C.POINTER(_capi.sm_create_opts), C.c_int32])
    assert sig["sm_create_opts_default"] == (None, [C.POINTER(_capi.sm_create_opts)])
    assert [f for f, _ in _capi.sm_create_opts._fields_] == ["struct_size", "so_float_minima"]
    assert re.search(r"typedef struct sm_create_opts \{\s*uint32_t struct_size;[^}]*int32_t so_float_minima;[^}]*\} sm_create_opts;", hdr)
    assert _capi.default_params(15, 32, 32).struct_size == C.sizeof(_capi.sm_params) == 216
    assert "sgm / WTA only" not in hdr


# ---- the facades ---------------------------------------------------------------------------------------------

def test_so_needs_float_minima_is_validates_rule():
    """The facades' automatic setting is exactly what sm_create refuses for the sake of so's unsigned minima."""
    for agg in ("none", "CBCA", "GF", "NL", "FIF", "AWS", "BF", "GFNL"):
        for cost in _capi.COST_METHODS:
            for trunc in (20.0, 1e-30, 0.1, 0.5, 1024.0, 1025.0):
                for opt in ("so", "sgm", ""):
                    p = _capi.default_params(15, 32, 32, aggregation=agg, cost_method=cost, optimization=opt, ad_trunc_ad=trunc)
                    lib, ctx, st = _create(p)
                    msg = lib.sm_last_error(ctx)
                    lib.sm_destroy(ctx)
                    refused = st == _capi.SM_EINVAL and (b"supports optimization sgm or WTA" in msg or b"with optimization so" in msg)
                    assert refused == _capi.so_needs_float_minima(p), (agg, cost, trunc, opt, msg)
                    if st == _capi.SM_EINVAL:
                        assert refused, msg


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    real = _capi.load()
    r.sm_params_default = real.sm_params_default          # host-only: fills the struct
    monkeypatch.setattr(_capi, "load", lambda: r)
    return r


def _created(rec):
    """[(entry point, sm_params, so_float_minima or None)] of the recorded creations."""
    out = []
    for name, args in rec.calls:
        if name == "sm_create":
            out.append((name, args[1]._obj, None))
        elif name == "sm_create_ex":
            assert args[2]._obj.struct_size == C.sizeof(_capi.sm_create_opts)
            out.append((name, args[1]._obj, args[2]._obj.so_float_minima))
    return out


def test_stereo_batch_chooses_the_entry_point(rec):
    def one(**kw):
        rec.calls.clear()
        sb = StereoBatch(15, 32, 40, 2, **kw)
        sb._ctx = None
        (made,) = _created(rec)
        return made

    assert one(optimization="so")[0] == "sm_create"
    assert one(optimization="sgm", aggregation="GF")[0] == "sm_create"
    for kw in (dict(aggregation="GF"), dict(aggregation="GFNL"), dict(aggregation="BF", cost_method="grad"),
               dict(aggregation="BF", cost_method="AD", ad_trunc_ad=0.1)):
        name, p, fm = one(optimization="so", **kw)
        assert (name, fm) == ("sm_create_ex", 1) and p.keep_final_volume == 0, kw
    assert one(optimization="so", aggregation="BF", cost_method="AD")[0] == "sm_create"
    # forced either way
    assert one(optimization="so", so_float_minima=True)[::2] == ("sm_create_ex", 1)
    assert one(optimization="so", aggregation="GF", so_float_minima=False)[0] == "sm_create"
    assert one(optimization="sgm", so_float_minima=True)[::2] == ("sm_create_ex", 1)
    assert one(optimization="so", aggregation="GF", so_float_minima=None)[::2] == ("sm_create_ex", 1)


def test_stereo_batch_keeps_the_volume_for_the_stages_that_read_it(rec):
    def keep(**kw):
        rec.calls.clear()
        sb = StereoBatch(15, 32, 40, 2, **kw)
        sb._ctx = None
        return _created(rec)[0][1].keep_final_volume

    assert keep(optimization="so", do_refine=1) == 0
    assert keep(optimization="so", do_refine=1, refine_ext=dict(do_bg_ipol=True)) == 0
    assert keep(optimization="so", do_refine=1, refine_ext=dict(do_pkr=True)) == 1
    assert keep(optimization="so", do_refine=1, refine_ext=dict(do_subpixel=True)) == 1
    assert keep(optimization="so", do_refine=1, refine_da=dict(on=True)) == 1
    assert keep(optimization="so", do_refine=1, refine_da=dict(canny_low=10)) == 1   # refine_da_config's `on` defaults to True
    assert keep(optimization="so", do_refine=1, refine_da=dict(on=False)) == 0
    assert keep(optimization="sgm", do_refine=1, refine_ext=dict(do_pkr=True)) == 0  # SGM keeps its path sum by itself
    assert keep(optimization="so", do_refine=1, refine_ext=dict(do_pkr=True), aggregation="GF") == 1
    assert keep(optimization="so", keep_final_volume=1) == 1
    assert [a[1:] for a in rec.named("sm_refine_ext_config")] == []


def test_stereo_matching_chooses_entry_point_and_volume(rec):
    cls = StereoMatching
    names = ("costcalculation", "aggregation", "optimization", "Do_refine", "Do_calPKR", "Do_subpixelEnhancement",
             "Do_discontinuityAdjust", "Do_bgIpol")
    saved = {k: getattr(cls, k) for k in names}
    z3, z1 = np.zeros((32, 40, 3), np.uint8), np.zeros((32, 40), np.uint8)

    def one(ctor=None, **statics):
        rec.calls.clear()
        for k in names:
            setattr(cls, k, saved[k])
        for k, v in statics.items():
            setattr(cls, k, v)
        sm = cls(z3, z3, z1, z1, param=cls.Parameters(15, 32, 40), **(ctor or {}))
        sm._ctx = None
        (made,) = _created(rec)
        return made[0], made[1].keep_final_volume, made[2]

    try:
        assert one(optimization="so", aggregation="CBCA") == ("sm_create", 0, None)
        assert one(optimization="so", aggregation="GF") == ("sm_create_ex", 0, 1)
        assert one(optimization="so", aggregation="GFNL") == ("sm_create_ex", 0, 1)
        assert one(optimization="so", aggregation="BF", costcalculation="grad") == ("sm_create_ex", 0, 1)
        assert one(optimization="so", aggregation="BF", costcalculation="censusGrad") == ("sm_create", 0, None)
        assert one(optimization="sgm", aggregation="GF") == ("sm_create", 0, None)
        assert one(dict(so_float_minima=True), optimization="so", aggregation="CBCA") == ("sm_create_ex", 0, 1)
        assert one(dict(so_float_minima=False), optimization="so", aggregation="GF") == ("sm_create", 0, None)
        for stage in ("Do_calPKR", "Do_subpixelEnhancement", "Do_discontinuityAdjust"):
            assert one(optimization="so", aggregation="CBCA", Do_refine=True, **{stage: True}) == ("sm_create", 1, None), stage
            assert one(optimization="so", aggregation="CBCA", Do_refine=False, **{stage: True}) == ("sm_create", 0, None), stage
            assert one(optimization="sgm", aggregation="CBCA", Do_refine=True, **{stage: True}) == ("sm_create", 0, None), stage
        assert one(optimization="so", aggregation="CBCA", Do_refine=True, Do_bgIpol=True) == ("sm_create", 0, None)
        assert one(optimization="so", aggregation="GF", Do_refine=True, Do_calPKR=True) == ("sm_create_ex", 1, 1)
        assert one(dict(keep_final_volume=True), optimization="so", aggregation="CBCA") == ("sm_create", 1, None)
    finally:
        for k, v in saved.items():
            setattr(cls, k, v)


def test_cpp_facade_source_and_docs():
    src = open(os.path.join(ROOT, "include", "stereo_matching.hpp")).read()
    for text in ("inline static int SO_FLOAT_MINIMA = -1;", "sm_create_ex(&ctx_, &p, &o, hip_device)", "p.keep_final_volume = 1;"):
        assert text in src, text
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 24." in design and "so_float_minima" in design and "so_first_min" in design
    for name in ("README.md", "INTEGRATION.md"):
        assert "so_float_minima" in open(os.path.join(ROOT, name)).read(), name


# ---- the restatement against the C oracle, on the crafted volumes -------------------------------------------

@pytest.fixture(scope="module")
def crafted(oracle):
    """{(H, W, D): (pair, the crafted volume for so / so_R2L)} and the same with H and W exchanged for so_T2D."""
    out = {}
    for H, W, D in CRAFTED:
        pair, v0, _ = volumes(oracle, H, W, D, 700 + H)
        out[(H, W, D)] = (pair, SC.craft(v0, 1000 + W))
        pair, v0, _ = volumes(oracle, W, H, D, 700 + H)
        out[(W, H, D)] = (pair, SC.craft(v0, 1000 + W, lines="cols"))
    return out


def test_first_min_c_is_the_loop():
    rng = np.random.default_rng(11)
    vals = np.array([np.nan, -np.inf, np.inf, -0.0, 0.0, 1.0, -1.0, 2.5, -2.5, 1e-45, -1e-45], np.float32)
    c = vals[rng.integers(0, len(vals), (4000, 6))]
    want = np.empty(len(c), np.int32)
    for k, row in enumerate(c):
        m, i = row[0], 0
        for d in range(1, len(row)):
            if row[d] < m:
                m, i = row[d], d
        want[k] = i
    np.testing.assert_array_equal(PF.first_min_c(c), want)
    assert (PF.first_min_unsigned(c) != want).any() and (PF.first_min_nan_dropping(c) != want).any()
    assert (PF.first_min_signed_zero(c) != want).any() and (np.argmin(c, axis=1) != want).any()
    # on volumes without NaN the two restatements agree
    f = rng.standard_normal((500, 9)).astype(np.float32)
    np.testing.assert_array_equal(PF.first_min_c(f), P._first_min(f))


@pytest.mark.parametrize("H,W,D", CRAFTED[:3] + CRAFTED[4:])
def test_so_equals_the_oracle_on_crafted_volumes(oracle, crafted, H, W, D):
    pair, vol = crafted[(H, W, D)]
    dp, acc = PF.so(vol, pair["lbgr"])
    rdp, racc = oracle_so(oracle, vol, pair["lbgr"])
    np.testing.assert_array_equal(dp, rdp)
    assert PF.same_floats(acc, racc)
    assert np.isnan(racc).any() and (racc[~np.isnan(racc)] < 0).any()


@pytest.mark.parametrize("H,W,D", CRAFTED[:3] + CRAFTED[4:])
def test_r2l_is_the_mirror_of_so_on_crafted_volumes(oracle, crafted, H, W, D):
    pair, vol = crafted[(H, W, D)]
    img = pair["lbgr"]
    dp, acc = PF.so_r2l(vol, img, *PF.SO_PN)
    rdp, racc = oracle_so(oracle, vol[:, ::-1], img[:, ::-1])
    np.testing.assert_array_equal(dp, rdp[:, ::-1])
    assert PF.same_floats(acc, racc[:, ::-1])


@pytest.mark.parametrize("H,W,D", CRAFTED[:3] + CRAFTED[4:])
def test_t2d_plain_is_the_transpose_of_so_on_crafted_volumes(oracle, crafted, H, W, D):
    pair, vol = crafted[(W, H, D)]
    img = pair["lbgr"]
    dp, acc = PF.so_t2d(vol, img, *PF.SO_PN, normalised=False)
    rdp, racc = oracle_so(oracle, vol.transpose(1, 0, 2), img.transpose(1, 0, 2))
    np.testing.assert_array_equal(dp, rdp.T)
    assert PF.same_floats(acc, racc.transpose(1, 0, 2))


def test_restatements_agree_on_finite_volumes(oracle):
    pair, v0, v1 = volumes(oracle, 26, 71, 32, 600)
    for a, b in ((P.so, PF.so), (P.so_r2l, PF.so_r2l), (P.so_t2d, PF.so_t2d)):
        for v in (v0, v1):
            x, y = a(v, pair["lbgr"]), b(v, pair["lbgr"])
            np.testing.assert_array_equal(x[0], y[0])
            assert x[1].tobytes() == y[1].tobytes()


@pytest.mark.parametrize("H,W,D", CRAFTED)
def test_crafted_volumes_are_not_vacuous(crafted, H, W, D):
    """(a), (b), (c) of so_float_cases.assert_not_vacuous, from the restatement alone, for all three variants."""
    assert SC.sizeable(W, H, D)
    pair, vol = crafted[(H, W, D)]
    nan = np.isnan(vol)
    assert nan[H // 2].all() and 0 < nan.all(axis=2).mean() < 0.2
    assert ((vol < 0) & ~nan).mean() > 0.3 and (np.signbit(vol) & (vol == 0)).any()
    for variant in ("so", "so_R2L"):
        print(H, W, D, variant, SC.assert_not_vacuous(variant, vol, pair["lbgr"]))
    pair, vol = crafted[(W, H, D)]
    assert np.isnan(vol[:, H // 2]).all()
    print(W, H, D, "so_T2D", SC.assert_not_vacuous("so_T2D", vol, pair["lbgr"]))


# ---- the end-to-end GF inputs -----------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,D,mode", [(26, 71, 32, 0), (26, 71, 32, 1), (12, 40, 16, 0)])
def test_gf_inputs_go_negative(oracle, H, W, D, mode):
    """tests/test_gpu_so_float.py's GF cases show something only where GF's costs are negative: through the oracle's
    guided filter, degenerate.signed_blocks with that file's seed has a negative cost at > 10 % of the pixels (and
    make_pair's texture at none, which is why it is not used there)."""
    import degenerate
    pair = degenerate.signed_blocks(H, W, 5)
    agg = oracle.run(pair, oracle.config(H, W, D - 1, aggregation=2, gf_mode=mode, optimization=0), dumps=True)["agg"]
    share = float((agg.min(axis=2) < 0).mean())
    print(f"GF {H}x{W}x{D} gf_mode {mode}: a negative cost at {100 * share:.1f} % of the pixels")
    assert not np.isnan(agg).any() and share > 0.10

