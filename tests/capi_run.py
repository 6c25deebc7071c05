"""One pair through the reference-ordered C ABI, every stage read back (a plain test helper).

run_ctx() follows main_.cpp's order -- sm_set_images, sm_cost_calculate, sm_solve_all,
sm_disp_optimize, sm_refine -- with any sm_params field overridden, and returns what each stage
left: the aggregated volume(s), the final volume (keep_final_volume), DP[0] before refine(),
DP[1] where it exists and the refined map.
"""
import ctypes as C

import numpy as np

from mystereomatching_amd import _capi

KEYS = ("lbgr", "rbgr", "lgray", "rgray")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits_equal(got, want, err_msg=""):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=err_msg)


def assert_bits_equal_nan(got, want, err_msg=""):
    """Bit equality that tolerates the one thing two IEEE machines may disagree on: which NaN.
    The NaN masks must be equal and the uint32 patterns equal wherever the value is not NaN
    (x86 produces the negative default NaN 0xffc00000, the GPU 0x7fc00000).  Without a NaN in
    either array this is exactly assert_bits_equal."""
    got = np.ascontiguousarray(got, np.float32)
    want = np.ascontiguousarray(want, np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(gn, wn, err_msg=f"{err_msg} (NaN mask)")
    np.testing.assert_array_equal(np.where(gn, 0, bits(got)), np.where(wn, 0, bits(want)), err_msg=err_msg)


class Ctx:
    """A C-ABI context that is destroyed on exit."""

    def __init__(self, md, H, W, **params):
        self.lib = _capi.load()
        self.shape = (H, W, md + 1)
        self.p = _capi.default_params(md, H, W, **params)
        self.ctx = C.c_void_p()
        _capi.check(self.lib, self.ctx, self.lib.sm_create(C.byref(self.ctx), C.byref(self.p), 0), "sm_create")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.sm_destroy(self.ctx)
        return False

    def call(self, name, *args):
        _capi.check(self.lib, self.ctx, getattr(self.lib, name)(self.ctx, *args), name)

    def set_images(self, pair):
        H, W, _ = self.shape
        a = {k: np.ascontiguousarray(pair[k]) for k in KEYS}
        self.call("sm_set_images", _capi.ptr(a["lbgr"]), _capi.ptr(a["rbgr"]), W * 3, _capi.ptr(a["lgray"]),
                  _capi.ptr(a["rgray"]), W)

    def volume(self, view=0):
        out = np.empty(self.shape, np.float32)
        self.call("sm_get_volume", view, _capi.ptr(out))
        return out

    def disp(self, view=0):
        out = np.empty(self.shape[:2], np.int16)
        self.call("sm_get_disp", view, _capi.ptr(out))
        return out

    def set_disp(self, view, m):
        self.call("sm_set_disp", view, _capi.ptr(np.ascontiguousarray(m, np.int16)))

    def optimize(self):
        out = np.empty(self.shape[:2], np.int16)
        self.call("sm_disp_optimize", _capi.ptr(out))
        return out

    def refine(self):
        out = np.empty(self.shape[:2], np.int16)
        self.call("sm_refine", _capi.ptr(out))
        return out


def run_ctx(pair, md, reg_lambda=0.3, right_volume=False, **params):
    """dict(agg, [agg_right], final, disp_raw, [disp_right], [disp]) of one pair; params are
    sm_params fields (keep_final_volume is set).  DP[1] is read with do_refine or "so"."""
    H, W = pair["lgray"].shape
    params.setdefault("keep_final_volume", 1)
    with Ctx(md, H, W, **params) as c:
        c.set_images(pair)
        c.call("sm_cost_calculate")
        out = {"agg": c.volume(0)}
        if right_volume:
            out["agg_right"] = c.volume(1)
        c.call("sm_solve_all", 1, reg_lambda)
        out["disp_raw"] = c.optimize()
        out["final"] = c.volume(0)
        if c.p.do_refine or c.p.optimization == 2:
            out["disp_right"] = c.disp(1)
        if c.p.do_refine:
            out["disp"] = c.refine()
    return out
