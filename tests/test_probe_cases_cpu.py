"""The probe groups' inputs, held to their non-vacuity conditions on the
reference alone (tests/probe_cases.py): a generator that drifts
into easy cases fails here, not silently on the GPU.  No GPU.
"""
import numpy as np

import oracle
import probe_cases as pc


def test_division_covers_every_side():
    g = pc.division()
    assert len(g["n"]) == pc.MAX_SIDE * 4 * 11 <= 3_000_000
    d = g["d_int"]
    assert np.array_equal(np.unique(d), np.arange(1, pc.MAX_SIDE + 1))
    # n = x + r with x in {0, 1, d // 2, d - 1} and r a multiple of 2^-32 below 1
    units = g["n"] * 2.0 ** 32
    assert np.all(units == np.floor(units)) and np.all(g["n"] >= 0)
    # an inexact quotient per side.  A power of two divides exactly whatever n is
    # (no quotient here is subnormal), so the condition is on every other side:
    # all 65519 of them.
    per_d = np.zeros(pc.MAX_SIDE + 1, bool)
    np.logical_or.at(per_d, d, g["inexact"])
    pow2 = (np.arange(pc.MAX_SIDE + 1) & (np.arange(pc.MAX_SIDE + 1) - 1)) == 0
    assert np.all(per_d[1:][~pow2[1:]])
    assert not np.any(per_d[pow2])
    # the exactness rule itself, on a sample, in exact arithmetic
    from fractions import Fraction

    for i in np.random.default_rng(1).integers(0, len(d), 300):
        exact = Fraction(float(g["q"][i])) * int(d[i]) == Fraction(float(g["n"][i]))
        assert exact != bool(g["inexact"][i])


def test_root_range_fills_the_undecided_band():
    g = pc.root_range()
    band = g["band"]
    assert band.sum() >= 1000
    assert (band & (g["out"] == 0)).sum() >= 300
    assert (band & (g["out"] == 1)).sum() >= 300
    # the edges the issue names
    num, a = g["num"], g["a"]
    assert np.isinf(g["tmax"]).any() and np.isnan(num).any() and np.isnan(a).any() and np.isinf(num).any()
    assert np.isinf(a).any() and (a == 0).any() and ((a > 0) & (a < 2.0 ** -1022)).any()
    assert ((num == 0) & np.signbit(num)).any() and ((num == 0) & ~np.signbit(num)).any()
    # both bounds carry band cases, and a spans 2^-60 .. 2^60
    with np.errstate(all="ignore"):
        lo = band & (np.abs(g["q"] - g["tmin"]) <= 2.0 ** -40 * np.abs(g["q"]))
        hi = band & (np.abs(g["q"] - g["tmax"]) <= 2.0 ** -40 * np.abs(g["q"]))
    assert lo.sum() >= 300 and hi.sum() >= 300
    assert a[band].min() <= 2.0 ** -59 and a[band].max() >= 2.0 ** 59


def test_unit_ball_fills_the_shell():
    g = pc.unit_ball()
    off = g["off"]
    shell = np.abs(off) <= 2.0 ** -16
    assert shell.sum() >= 2000
    assert (shell & (off < 0)).sum() >= 500 and (shell & (off > 0)).sum() >= 500
    # within 2^-31 of 1, either side; exactly 1 (rejected); the screen's own limits
    ex = g["exact_off"]
    near = np.array([abs(int(v)) <= (1 << 31) for v in ex])
    assert (near & (off < 0)).sum() >= 500 and (near & (off > 0)).sum() >= 500
    on = np.array([int(v) == 0 for v in ex])
    assert on.sum() >= 3 and not g["accept"][on].any()
    u = g["u"]
    for t in ((0, 2 ** 31, 2 ** 31), (2 ** 31, 0, 2 ** 31), (2 ** 31, 2 ** 31, 0)):
        assert (u == np.array(t, np.uint32)).all(1).any()
    for centre in (1 + 2.0 ** -16 * (1 + 2.0 ** -4), 1 + 2.0 ** -16 * (1 - 2.0 ** -4), 1 - 2.0 ** -16 * (1 + 2.0 ** -4),
                   1 - 2.0 ** -16 * (1 - 2.0 ** -4), 1 + 2.0 ** -18, 1 - 2.0 ** -18, 1 + 2.0 ** -14, 1 - 2.0 ** -14):
        assert (np.abs(off - (centre - 1)) <= 2.0 ** -29).sum() >= 300, centre
    assert len(u) - g["n_constructed"] == 100000
    # the decision is the rounded sum's: within a few 2^-53 of 1 it differs from the exact length's, and
    # the cases hold such triples; nowhere else
    odd = ((off < 0) & (g["accept"] == 0)) | ((off >= 0) & (g["accept"] == 1))
    assert odd[~on].any() and np.all(np.abs(off[odd]) <= 2.0 ** -51)
    assert (np.abs(off) <= 2.0 ** -56).sum() >= 100
    # the screen's worst case: every low byte 0x7f, or every one 0x81, near the sphere
    for low in (0x7F, 0x81):
        assert (((u & 0xFF) == low).all(1) & (np.abs(off) <= 2.0 ** -22)).sum() >= 400


def test_sphere_query_cases():
    g = pc.sphere_query()
    w = g["which"]
    for k in (0, 1, 2):
        assert (w == k).sum() >= 500, (k, (w == k).sum())
    # the restatement that names the root is the oracle's Sphere.Hit on every case
    assert np.array_equal(w > 0, g["oracle_ok"])
    assert pc.same_bits(np.where(w > 0, g["ref_t"], 0.0), g["oracle_t"]).all()
    # grazing on both sides, roots at the bounds, a zero direction, the ground sphere, scaled directions
    disc = g["disc"]
    a = pc._dot(g["d"], g["d"])
    with np.errstate(all="ignore"):
        hb2 = disc / (a * g["radii"][g["sphere"]] ** 2)  # the discriminant against its own terms
    assert ((disc < 0) & (hb2 > -2.0 ** -40)).sum() >= 100 and ((disc >= 0) & (hb2 < 2.0 ** -40)).sum() >= 100
    assert g["band"].sum() >= 500
    assert (a == 0).sum() >= 10 and np.isnan(g["oracle_t"][a == 0]).any()
    ground = g["sphere"] == 2
    assert (ground & (w == 0)).sum() >= 100 and (ground & (w > 0)).sum() >= 100
    assert a.min() <= 2.0 ** -70 and a.max() >= 2.0 ** 70
    # an origin inside a sphere takes the second root
    oc = g["o"] - g["centers"][g["sphere"]]
    inside = pc._dot(oc, oc) < 0.5 * g["radii"][g["sphere"]] ** 2
    assert (inside & (w == 2)).sum() >= 200


def test_triangle_cases():
    g = pc.triangle_test()
    assert g["edge"].sum() >= 200
    for s in (1, 2, 3, 4):
        assert (g["stage"] == s).sum() >= 200, (s, (g["stage"] == s).sum())
    acc = g["stage"] == 0
    assert np.array_equal(acc, g["oracle_ok"])
    assert pc.same_bits(g["t"], g["oracle_t"]).all()
    u, v = g["u"], g["v"]
    assert (acc & (u == 0)).sum() >= 40 and (acc & (v == 0)).sum() >= 40 and (acc & (u + v == 1) & (u > 0)).sum() >= 40
    assert g["near_a"].sum() >= 100 and (g["near_a"] & (g["stage"] == 1)).any() and (g["near_a"] & (g["stage"] != 1)).any()
    assert g["near_t"].sum() >= 200
    # back faces and parallel rays
    V = g["verts"][g["tri"]]
    a = pc.ref_tri(V[:, 0], V[:, 1], V[:, 2], g["o"], g["d"], g["tmin"], g["tmax"])[4]
    assert (acc & (a < 0)).sum() >= 100 and (acc & (a > 0)).sum() >= 100 and (a == 0).sum() >= 100


def test_slab_cases():
    pairs = zero = 0
    for which in (0, 1):
        g = pc.slab(which)
        pairs += len(g["pairs"])
        zero += int(g["pair_zero"].sum())
        assert g["ray_kinds"]["at_tmax"] >= 50 and g["ray_kinds"]["thin"] >= 200
        # every accepted pair reaches the root through its ancestors
        assert (g["node"][:g["hit_cases"]] == 0).sum() == len(g["pairs"])
        assert len(g["node"]) <= 3_000_000
        ex = g["exact"]
        assert ex.any() and not ex.all()
    assert pc.slab(1)["flat"]["boxes"].size > 0 and (pc.slab(1)["box"] >= 0).any()
    assert pairs >= 20000, pairs
    assert zero >= 1000, zero


def test_go_scalar_cases():
    g = pc.go_scalars()
    x = g["x"][:g["n_pow"]]
    assert np.isnan(x).any() and (x == np.inf).any() and (x == -np.inf).any()
    assert ((x == 0) & np.signbit(x)).any() and ((x == 0) & ~np.signbit(x)).any()
    fin = np.isfinite(x) & (x != 0)
    assert np.abs(x[fin]).min() == 2.0 ** -53 and np.abs(x[fin]).max() == 1000.0
    assert (x[fin] < 0).sum() >= 1000 and (x[fin] > 0).sum() >= 1000
    # the expected powers are Go's: spot values
    assert oracle.go_pow(2.0, 5.0) == 32.0 and oracle.go_pow(-2.0, 5.0) == -32.0
    # the amd64 rule, spelled out once more for the table's entries that are in range
    for f, b in pc.GO_U8:
        if f == f and abs(f) < 2.0 ** 63:
            assert int(f) % 256 == b, (f, b)
        else:
            assert b == 0


def test_tonemap_thresholds_and_margin():
    g = pc.tonemap()
    th = g["thresholds"]
    assert len(th) == 255 and np.all(np.diff(th.astype(np.int64)) > 0)
    # the pair of every byte, and the margin of its nearer float, in binary64 ulps of k
    margins = []
    for k, p in zip(range(1, 256), th):
        below, at = pc._f32(p - 1), pc._f32(p)
        assert pc.oracle_byte(below) == k - 1 and pc.oracle_byte(at) == k
        if k <= 254:
            ulp = np.spacing(float(k))
            near = min(abs(oracle.tonemap((float(x), 0, 0))[0] * 255 - k) for x in (below, at))
            margins.append(near / ulp)
    assert min(margins) >= 2.0 ** 16, min(margins)
    assert int(np.argmin(margins)) + 1 == 254 and th[253] == 1083714120
    assert th[254] == 1108431690  # saturation: 1 - exp(-m) = 1 - 2^-53 from here on
    # host and oracle agree on the edge rows; every byte value occurs
    assert np.array_equal(g["host"][:g["n_edge"]], g["oracle"])
    assert len(np.unique(g["oracle"])) == 256
    assert np.isnan(g["rgb"]).any() and (g["rgb"] < 0).any() and np.isinf(g["rgb"]).any()


def test_scatter_cases():
    g = pc.scatter()
    kinds = [m["type"] for m in pc.MATERIALS]
    assert set(kinds) == {"lambertian", "metal", "shiny", "perfectmirror", "glass", "dielectric", "diffuselight"}
    mat = g["mat"][g["case"]]
    nd_dot_n = pc._dot(g["out"][:, :3], g["N"][g["case"]])
    for kind in ("glass", "dielectric"):
        m = np.isin(mat, [i for i, k in enumerate(kinds) if k == kind])
        forced = m & (g["draws"] == 0)
        drawn_reflect = m & (g["draws"] == 1) & (nd_dot_n > 0)
        refract = m & (g["draws"] == 1) & (nd_dot_n < 0)
        assert forced.sum() >= 300 and drawn_reflect.sum() >= 300 and refract.sum() >= 300, kind
        # a forced reflection is the one with ratio * sin > 1
        rs = g["ratio_sin"][g["case"]]
        assert np.array_equal(forced, m & (rs > 1.0))
    # the critical angle from both sides, within ulps; the clamp; the streams
    rs = g["ratio_sin"]
    assert ((rs > 1) & (rs <= 1 + 2.0 ** -50)).sum() >= 20 and ((rs <= 1) & (rs >= 1 - 2.0 ** -50)).sum() >= 20
    assert (g["raw_cos"] > 1).sum() >= 100
    assert len(g["state"]) == len(g["mat"]) * pc.STREAMS
    # the states are the spec's: the first raw draw of a few streams, against the oracle
    for i in (0, 1, 63, 64, 1000):
        _, raw = oracle.rng_draws(pc.SEED, int(g["case"][i]), i % pc.STREAMS, 1)
        x = int(g["state"][i])
        xs = (((x >> 18) ^ x) >> 27) & 0xFFFFFFFF
        rot = x >> 59
        assert int(raw[0]) == ((xs >> rot) | (xs << ((32 - rot) & 31))) & 0xFFFFFFFF
    # draws: none where no point is drawn, one per decision, three per try of the rejection loop
    for i, m in enumerate(pc.MATERIALS):
        dr = g["draws"][mat == i]
        rough = m.get("roughness", 0.0)
        if m["type"] == "lambertian" or (m["type"] in ("metal", "perfectmirror") and rough > 0.001) or \
                (m["type"] == "shiny" and rough > 0):
            assert dr.min() >= 3 and np.all(dr % 3 == 0) and dr.max() > 3
        elif m["type"] in ("glass", "dielectric"):
            assert set(dr.tolist()) <= {0, 1}
        else:
            assert not dr.any()
    light = mat == kinds.index("diffuselight")
    assert not g["ok"][light].any() and g["ok"][~light].all()
