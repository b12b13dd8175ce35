"""The device functions of csrc/rt_device.h, one at a time, against plain
references (tests/probe_cases.py; the probes: tests/c/device_probe.hip, built
by `make probe` with the product's flags).

Every other GPU test renders an image, which decides a shortcut of
rt_device.h only where one of its rays happens to land.  Here each shortcut
runs on the edges of its own argument: one launch per group, one lane per case,
every comparison on bits or integers (any NaN equal to any NaN).  The one
group that is not an equality is the slab tests', which are conservative by
design: no true hit may be rejected, and how often they pass a box that an
exact test rejects is printed, not asserted.
"""
import numpy as np
import pytest

import probe_cases as pc

pytestmark = pytest.mark.gpu


def _run(name, ins, outs, head=()):
    """One probe launch: `ins` numpy arrays -> device, `outs` [(dtype, shape)]
    allocated there and poisoned, all passed after `head`; returns the outputs."""
    import torch

    L = pc.probe_lib()  # (a missing library raises: a failure, not a skip)
    count = len(ins[-1]) if ins[-1].ndim == 1 else ins[-1].shape[0]
    dev_in = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda() for a in ins]
    dev_out = []
    for dt, shape in outs:
        nbytes = int(np.prod(shape)) * np.dtype(dt).itemsize
        dev_out.append(torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda"))
    args = list(head) + [t.data_ptr() for t in dev_in + dev_out] + [count, None]
    torch.cuda.synchronize()
    rc = getattr(L, name)(*args)
    assert rc == 0, f"{name}: hipError {rc}"
    torch.cuda.synchronize()
    return [t.cpu().numpy().view(dt).reshape(shape) for t, (dt, shape) in zip(dev_out, outs)]


def _records(arr):
    """A record array of the product on the device: (tensor to keep alive, pointer, count)."""
    import torch

    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    t = torch.from_numpy(raw if raw.size else np.zeros(16, np.uint8)).cuda()
    return t, t.data_ptr(), len(arr)


def _mismatch(ok, *cols):
    bad = np.flatnonzero(~ok)
    return f"{len(bad)} of {len(ok)} cases differ; first: " + "; ".join(
        f"#{i}: " + ", ".join(repr(c[i]) for c in cols) for i in bad[:5])


def test_div_by_is_the_ieee_quotient():
    g = pc.division()
    n = len(g["n"])
    (q,) = _run("rtp_div", [g["n"], g["d"]], [(np.float64, (n,))])
    ok = q.view(np.uint64) == g["q"].view(np.uint64)
    assert ok.all(), _mismatch(ok, g["n"], g["d"], q, g["q"])


def test_root_out_is_the_exact_quotients_answer():
    g = pc.root_range()
    n = len(g["num"])
    (out,) = _run("rtp_root_out", [g["num"], g["a"], g["tmin"], g["tmax"]], [(np.int32, (n,))])
    ok = out == g["out"]
    assert ok.all(), _mismatch(ok, g["num"], g["a"], g["tmin"], g["tmax"], out, g["out"])


def test_unit_ball_accept_is_the_binary64_decision():
    g = pc.unit_ball()
    n = len(g["u"])
    acc, pt = _run("rtp_unit_ball", [g["u"]], [(np.int32, (n,)), (np.float64, (n, 3))])
    ok = acc == g["accept"]
    assert ok.all(), _mismatch(ok, g["u"], g["off"], acc, g["accept"])
    okp = (pt.view(np.uint64) == g["point"].view(np.uint64)).all(1)
    assert okp.all(), _mismatch(okp, g["u"], pt, g["point"])


def test_sphere_query_takes_the_oracles_root():
    g = pc.sphere_query()
    flat = pc.flatten(pc.sphere_scene())
    S = flat["spheres"]
    # the product's records are the cases' spheres, found by their object index
    where = np.full(len(g["radii"]), -1, np.int32)
    where[S["obj"]] = np.arange(len(S), dtype=np.int32)
    assert (where >= 0).all() and np.array_equal(S["c"][where], g["centers"]) and np.array_equal(S["r"][where], g["radii"])
    keep, ptr, ns = _records(S)
    n = len(g["sphere"])
    which, t = _run("rtp_sphere_query", [where[g["sphere"]], g["o"], g["d"], g["tmin"], g["tmax"]],
                    [(np.int32, (n,)), (np.float64, (n,))], head=(ptr, ns))
    ok = (which == g["which"]) & ((which > 0) == g["oracle_ok"])
    assert ok.all(), _mismatch(ok, g["sphere"], g["o"], g["d"], g["tmax"], which, g["which"])
    okt = pc.same_bits(t, g["oracle_t"])
    assert okt.all(), _mismatch(okt, g["sphere"], g["o"], g["d"], g["tmax"], t, g["oracle_t"])


def test_tri_test_is_triangle_hit():
    g = pc.triangle_test()
    flat = pc.flatten(pc.triangle_scene())
    T = flat["tris"]
    # the product's triangle records, in the order of oracle.cube_triangles
    V = g["verts"]
    assert len(T) == len(V) and np.array_equal(T["v0"], V[:, 0])
    assert np.array_equal(T["e1"], V[:, 1] - V[:, 0]) and np.array_equal(T["e2"], V[:, 2] - V[:, 0])
    keep, ptr, nt = _records(T)
    n = len(g["tri"])
    hit, tuv = _run("rtp_tri_test", [g["tri"], g["o"], g["d"], g["tmin"], g["tmax"]],
                    [(np.int32, (n,)), (np.float64, (n, 3))], head=(ptr, nt))
    ok = (hit == (g["stage"] == 0)) & ((hit == 1) == g["oracle_ok"])
    assert ok.all(), _mismatch(ok, g["tri"], g["o"], g["d"], g["tmin"], g["tmax"], hit, g["stage"])
    okt = pc.same_bits(tuv[:, 0], g["oracle_t"]) & pc.same_bits(tuv[:, 1], g["u"]) & pc.same_bits(tuv[:, 2], g["v"])
    assert okt.all(), _mismatch(okt, g["tri"], g["o"], g["d"], tuv, g["oracle_t"], g["u"], g["v"])


SLAB_BITS = {"box_hit/inv_dir": 1, "box_hit/inv_dir_fast": 2, "box_hit32/inv_dir": 4, "box_hit32/inv_dir_fast": 8}


@pytest.mark.parametrize("which", [0, 1], ids=["sphere_field", "spheres_and_cubes"])
def test_slab_tests_reject_no_true_hit(which, record_property):
    g = pc.slab(which)
    flat = g["flat"]
    keep_n, pn, nn = _records(flat["nodes"])
    keep_b, pb, nb = _records(flat["boxes"])
    n = len(g["node"])
    (out,) = _run("rtp_slab", [g["node"], g["box"], g["o"], g["d"], g["tmin"], g["tmax"]], [(np.int32, (n,))],
                  head=(pn, nn, pb, nb))
    assert (out >= 0).all()
    hit = np.arange(n) < g["hit_cases"]  # (ray, node) of a pair the oracle's hit function accepts
    root = g["node"] == 0
    # every box on the way to a true hit passes the binary32 tests, the root the binary64 one too
    for name in ("box_hit32/inv_dir", "box_hit32/inv_dir_fast"):
        ok = ~hit | ((out & SLAB_BITS[name]) != 0)
        assert ok.all(), name + ": " + _mismatch(ok, g["node"], g["o"], g["d"], g["tmax"], out)
    for name in ("box_hit/inv_dir", "box_hit/inv_dir_fast"):
        ok = ~(hit & root) | ((out & SLAB_BITS[name]) != 0)
        assert ok.all(), name + ": " + _mismatch(ok, g["node"], g["o"], g["d"], g["tmax"], out)
    cube = hit & (g["box"] >= 0)
    ok = ~cube | ((out & 16) != 0)
    assert ok.all(), "ray_box: " + _mismatch(ok, g["box"], g["o"], g["d"], g["tmax"], out)
    if which == 1:
        assert cube.any()
    # the sample against every node: what the exact test on the unpadded bounds accepts, every test
    # accepts; the share of the boxes they pass that it rejects is the price of the margins (recorded)
    ex = g["exact"]
    smp = out[g["hit_cases"]:]
    for name, bit in SLAB_BITS.items():
        passed = (smp & bit) != 0
        ok = ~ex | passed
        assert ok.all(), name + " rejects a box the exact test accepts: " + _mismatch(
            ok, g["node"][g["hit_cases"]:], g["o"][g["hit_cases"]:], g["d"][g["hit_cases"]:])
        share = float((passed & ~ex).sum()) / max(1, int(passed.sum()))
        record_property(f"false_positive_share[{name}]", share)
        print(f"slab[{which}] {name}: passed {int(passed.sum())} of {len(smp)} boxes, "
              f"{int((passed & ~ex).sum())} of them rejected by the exact test (share {share:.4f})")


def test_go_scalar_semantics():
    g = pc.go_scalars()
    n = len(g["x"])
    out, _ = _run("rtp_scalar", [g["x"], g["y"]], [(np.float64, (n, 10)), (np.uint32, (n,))])
    names = ["pow_n<5>", "pow_n<2>", "gmax0", "gmin1_first", "gmin_x1", "clamp01", "go_max2", "go_min2",
             "go_max2 (swapped)", "go_min2 (swapped)"]
    for k, name in enumerate(names):
        rows = slice(0, g["n_pow"]) if k < 2 else slice(None)  # the powers over their callers' domain
        ok = pc.same_bits(out[rows, k], g["expected"][rows, k])
        assert ok.all(), name + ": " + _mismatch(ok, g["x"][rows], g["y"][rows], out[rows, k], g["expected"][rows, k])


def test_go_u8_is_amd64_truncation():
    f = np.array([v for v, _ in pc.GO_U8])
    want = np.array([b for _, b in pc.GO_U8], np.uint32)
    _, u8 = _run("rtp_scalar", [f, np.zeros_like(f)], [(np.float64, (len(f), 10)), (np.uint32, (len(f),))])
    ok = u8 == want
    assert ok.all(), _mismatch(ok, f, u8, want)


def test_tonemap_bytes():
    g = pc.tonemap()
    n = len(g["rgb"])
    (px,) = _run("rtp_tonemap", [g["rgb"]], [(np.uint32, (n,))])
    got = np.stack([px & 0xFF, (px >> 8) & 0xFF, (px >> 16) & 0xFF], 1).astype(np.uint8)
    assert ((px >> 24) == 255).all()
    ne = g["n_edge"]
    ok = (got[:ne] == g["oracle"]).all(1)  # every byte threshold, every channel, against the oracle
    assert ok.all(), _mismatch(ok, g["rgb"][:ne], got[:ne], g["oracle"])
    ok = (got == g["host"]).all(1)         # everything against the host's toneMap + ToRGB
    assert ok.all(), _mismatch(ok, g["rgb"], got, g["host"])


def test_scatter_is_material_scatter():
    g = pc.scatter()
    flat = pc.flatten(pc.scatter_scene())
    S = flat["spheres"]
    mat_of = np.zeros(len(pc.MATERIALS), np.int32)  # the DMat of material i: its sphere's
    mat_of[S["obj"]] = S["mat"]
    keep, ptr, nm = _records(flat["mats"])
    case = g["case"]
    n = len(case)
    ok_d, out, state = _run("rtp_scatter",
                            [mat_of[g["mat"]][case], g["d"][case], g["N"][case], g["front"][case], g["state"]],
                            [(np.int32, (n,)), (np.float64, (n, 6)), (np.uint64, (n,))], head=(ptr, nm))
    ok = ok_d == g["ok"]
    assert ok.all(), _mismatch(ok, g["mat"][case], ok_d, g["ok"])
    # direction and attenuation, bit for bit (what a material that does not scatter leaves is not read)
    sc = g["ok"] != 0
    okv = pc.same_bits(out, g["out"]).all(1) | ~sc
    assert okv.all(), _mismatch(okv, g["mat"][case], g["d"][case], g["N"][case], g["front"][case], out, g["out"])
    # the draws consumed: the stream stands where the oracle's count puts it
    want = np.array([pc.advance(int(x), int(k)) for x, k in zip(g["state"], g["draws"])], np.uint64)
    oks = state == want
    assert oks.all(), _mismatch(oks, g["mat"][case], g["draws"])
