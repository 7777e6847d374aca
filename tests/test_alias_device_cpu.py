"""The alias table of ZR_ALIAS_BUILD_DEVICE as include/zr_alias.h states it, on the host (tests/aliasmath/libzal.so: the functions zr_tu_alias.hip compiles
for the device), against the host Vose build (api.alias_table_build) and float64.  No GPU.

Measured by test_table_is_valid_within_the_bound, max of |q - p| / (2^-21 p + 2^-30 / n), <= 1 required.  Over the 50 inputs of the set: the header's
table 0.2855 (one_zero, n = 4097; span sits at 0.25 for every n: its 2^-40 lights get the one unit a non-zero power is owed), the host Vose table 154.6
on the same input -- its residual chain carries the float rounding of every step into the last heavy light, so it leaves the bound from a few hundred
lights on (13.0 at one_zero n = 1000, 121.5 at span n = 4097).  Over cases.LARGE_CASES, where one weight passes 2^48: the header's table 0.0487 (one_heavy,
n = 100003), 0.1094 / 0.1505 (one light with a fifth of the power, n = 100000 / 40000), 0.2293 (log_uniform, n = 100003); the host Vose table 1.06e9,
0.1094, 5.2e5, 56.0.  The assertion on the header's table is therefore unconditional.
"""
import ctypes as C
import types

import numpy as np
import pytest

from tests.aliasmath import cases, zal
from zetaray_amd import api

CASES = cases.all_cases() + list(cases.LARGE_CASES)
_cache = {}


def _tables(kind, n):
    """(powers, the header's table, the host Vose table), computed once per input"""
    if (kind, n) not in _cache:
        p = cases.powers(kind, n)
        p.setflags(write=False)
        _cache[kind, n] = (p, zal.build(p), api.alias_table_build(p))
    return _cache[kind, n]


def _ids(c):
    return "%s-%d" % c


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_cached_p_orig_is_the_host_builds(case):
    p, dev, host = _tables(*case)
    assert np.array_equal(dev["cached_p_orig"].view(np.uint32), host["cached_p_orig"].view(np.uint32))


def test_kahan_sum_is_the_references_lane_order():
    # the lanes matter: a sum whose serial and eight-lane Kahan results differ in the last bit
    rng = np.random.default_rng(7)
    for n in (16, 31, 32, 1000, 4097):
        p = rng.uniform(0.0, 1.0, n).astype(np.float32) * np.exp2(rng.integers(-20, 20, n)).astype(np.float32)
        host = api.alias_table_build(p)
        # cached_p_orig[i] = (p[i] * (n / sum)) * (1 / n): recompute it from the header's sum
        s = np.float32(zal.lib().zal_kahan_sum(p.ctypes.data, n))
        want = (p * (np.float32(n) / s)) * (np.float32(1.0) / np.float32(n))
        assert np.array_equal(want.view(np.uint32), host["cached_p_orig"].view(np.uint32)), n


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_entries_are_well_formed(case):
    p, dev, _ = _tables(*case)
    n = len(p)
    assert (dev["alias"] < n).all()
    assert (dev["p_curr"] >= 0).all() and (dev["p_curr"] <= 1).all()
    assert np.array_equal(dev["cached_p_alias"].view(np.uint32), dev["cached_p_orig"][dev["alias"]].view(np.uint32))
    # only heavies are alias targets, and an entry with p_curr < 1 never aliases to itself
    other = dev["alias"] != np.arange(n)
    assert (dev["p_curr"][~other] == 1).all()


@pytest.mark.parametrize("n", cases.SIZES)
def test_equal_powers_alias_to_themselves(n):
    _, dev, _ = _tables("equal", n)
    assert np.array_equal(dev["alias"], np.arange(n, dtype=np.uint32))
    assert (dev["p_curr"] == 1).all()


@pytest.mark.parametrize("n", cases.SIZES[1:])
def test_zero_power_light_is_never_drawn(n):
    p, dev, _ = _tables("one_zero", n)
    z = n // 2
    assert p[z] == 0
    assert dev["p_curr"][z] == 0 and dev["cached_p_orig"][z] == 0
    assert not (np.delete(dev["alias"], z) == z).any()
    assert dev["alias"][z] != z
    assert cases.represented(dev)[z] == 0


def test_table_is_valid_within_the_bound(capsys):
    """|q_i - p_i| <= 2^-21 p_i + 2^-30 / n in float64 for every input; the host Vose table's figure on the same input is printed next to it"""
    worst = {"dev": (0.0, None), "host": (0.0, None)}
    failures = []
    with capsys.disabled():
        for case in CASES:
            p, dev, host = _tables(*case)
            ed, eh = cases.validity_excess(dev, p), cases.validity_excess(host, p)
            print("alias validity %-12s n=%-6d  header table: %8.4f of the bound   host Vose: %8.4f of the bound" % (case[0], case[1], ed, eh))
            if ed > worst["dev"][0]:
                worst["dev"] = (ed, case)
            if eh > worst["host"][0]:
                worst["host"] = (eh, case)
            if ed > 1.0:
                failures.append((case, ed, eh))
        print("alias validity max: header table %.4f (%s), host Vose %.4f (%s)" % (worst["dev"][0], worst["dev"][1], worst["host"][0], worst["host"][1]))
    assert not failures, failures


def test_weights_follow_the_quantisation_rule():
    for case in (("span", 1000), ("one_zero", 33), ("one_heavy", 4097)):
        p, dev, _ = _tables(*case)
        w = zal.weights(p)
        assert ((w == 0) == (p == 0)).all()
        probs = dev["cached_p_orig"].astype(np.float64) * len(p)
        assert (np.abs(w.astype(np.float64) - probs * 2.0 ** 32) <= np.maximum(1.0, probs * 2.0 ** 32 * 2.0 ** -23)).all()


def test_setter_refuses_bad_modes():
    L = api.lib()
    for mode in (-1, 2, 7):
        assert L.zr_scene_set_alias_build(None, mode) == 1          # ZR_ERR_INVALID_ARG
        assert b"mode" in L.zr_last_error()
    no_scene = types.SimpleNamespace(h=C.c_void_p())
    with pytest.raises(KeyError):
        api.Scene.set_alias_build(no_scene, "gpu")
    with pytest.raises(api.ZetaRayError) as e:
        api.Scene.set_alias_build(no_scene, 5)
    assert e.value.code == 1 and "mode 5" in str(e.value)
    assert api.ALIAS_BUILD_MODES == {"host": 0, "device": 1}
    assert {"zr_scene_set_alias_build", "zr_alias_table_build_device", "zr_pass_get_emissive_powers"} <= set(api.EXPORTS)
