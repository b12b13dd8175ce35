"""Degenerate scenes (shared by test_degenerate_cpu.py and test_gpu_degenerate.py).

Every kernel shortcut is exact only behind a guard for the inputs it cannot
handle ("Guards and the scenes that reach them"); these scenes
carry those inputs: negative and zero radii, coincident primitives, zero and
negative colours, out-of-range material parameters, flat cubes, the camera and
lights on surfaces, and non-finite lights, materials and geometry.

A scene is a dict {"camera", "objects", "lights"} for rtgo.Scene.from_python
(JSON cannot spell NaN or Inf).  A degenerate object or light carries a
"_fix" entry, which from_python ignores: None (drop it) or a dict of the fields
that make it ordinary.  repaired(scene) applies every fix: the oracle's image
of the repaired scene must differ from the scene's own, or a kernel that
ignored the degenerate inputs would pass (test_degenerate_cpu.py).

Layout of every scene: the reference's fixed camera at (0, 0.5, 6) looking down
-Z, a radius-1000 ground sphere whose top is y = -1, two ordinary lights.
"""
import copy
import json
import math

NAN, INF = float("nan"), float("inf")

CAM = {"position": [0, 0.5, 6], "aspectRatio": 1.5}
GROUND = {"type": "sphere", "position": [0, -1001, 0], "radius": 1000,
          "material": {"type": "lambertian", "color": [0.5, 0.5, 0.5]}}
LIGHTS = [{"position": [4, 6, 6], "color": [1, 1, 1], "intensity": 40.0},
          {"position": [-5, 3, 4], "color": [0.8, 0.8, 1], "intensity": 20.0}]

LAMB = {"type": "lambertian", "color": [0.6, 0.5, 0.4]}
RED = {"type": "lambertian", "color": [0.8, 0.2, 0.2]}
GREEN = {"type": "lambertian", "color": [0.2, 0.7, 0.3]}
BLUE = {"type": "lambertian", "color": [0.2, 0.3, 0.8]}
METAL = {"type": "metal", "color": [0.9, 0.8, 0.7], "roughness": 0.1, "metallic": 0.9}
ROUGH = {"type": "metal", "color": [0.9, 0.6, 0.3], "roughness": 0.4, "metallic": 0.7, "specular": 0.8}
MIRROR = {"type": "perfectmirror", "color": [0.9, 0.9, 0.9], "roughness": 0.0}
GLASS = {"type": "glass", "color": [0.9, 0.95, 1.0], "refractionIndex": 1.5}
GLASS2 = {"type": "glass", "color": [1.0, 0.7, 0.7], "refractionIndex": 1.3}
DIEL = {"type": "dielectric", "refractionIndex": 1.33}


def sph(p, r, m, fix="none"):
    o = {"type": "sphere", "position": list(p), "radius": r, "material": m}
    if fix != "none":
        o["_fix"] = fix
    return o


def cube(p, s, m, fix="none"):
    o = {"type": "cube", "position": list(p), "size": list(s), "material": m}
    if fix != "none":
        o["_fix"] = fix
    return o


def light(p, c, i, fix="none"):
    li = {"position": list(p), "color": list(c), "intensity": i}
    if fix != "none":
        li["_fix"] = fix
    return li


def scene(objects, lights=None, camera=None):
    return {"camera": copy.deepcopy(camera or CAM), "objects": [copy.deepcopy(GROUND)] + objects,
            "lights": copy.deepcopy(LIGHTS) + (lights or [])}


def _strip(items, fix):
    out = []
    for it in items:
        it = copy.deepcopy(it)
        f = it.pop("_fix", "none")
        if fix and f is None:
            continue
        if fix and f != "none":
            it.update(copy.deepcopy(f))
        out.append(it)
    return out


def clean(sc):
    """The scene without its "_fix" entries (for json.dumps)."""
    return {"camera": copy.deepcopy(sc["camera"]), "objects": _strip(sc["objects"], False),
            "lights": _strip(sc["lights"], False)}


def repaired(sc):
    """The scene with every degenerate object / light dropped or made ordinary."""
    return {"camera": copy.deepcopy(sc["camera"]), "objects": _strip(sc["objects"], True),
            "lights": _strip(sc["lights"], True)}


def spheres_only(sc):
    out = copy.deepcopy(sc)
    out["objects"] = [o for o in out["objects"] if o["type"] == "sphere"]
    return out


def is_finite(sc):
    def walk(v):
        if isinstance(v, dict):
            return all(walk(x) for x in v.values())
        if isinstance(v, (list, tuple)):
            return all(walk(x) for x in v)
        return not isinstance(v, float) or math.isfinite(v)

    return walk(clean(sc))


def to_json(sc):
    return json.dumps(clean(sc), allow_nan=False)


def load(rtgo, sc):
    sc = clean(sc)
    return rtgo.Scene.from_python(sc["camera"], sc["objects"], sc["lights"])


def fixture_text(rtgo):
    """Every scene as the C ABI sees it (rt_scene, loader defaults applied), one
    record per line, numbers in repr() form: the shortest decimal that reads
    back to the same binary64, "nan", "inf" (all of which strtod reads).  The
    sanitizer driver (tests/c/sanitize_driver.cpp) reads it from
    tests/golden/degenerate_scenes.txt (written by tests/golden/make_degenerate.py)."""
    def num(vals):
        return " ".join(repr(float(v)) for v in vals)

    lines = ["# name / camera / objects / lights of tests/degenerate_cases.py (make_degenerate.py)"]
    for name, sc in SCENES.items():
        v = load(rtgo, sc).view
        c = v.camera
        lines.append(f"scene {name}")
        lines.append("camera " + num(list(c.position) + list(c.look_at) + list(c.up) + [c.fov, c.aspect_ratio]))
        for i in range(v.num_objects):
            o = v.objects[i]
            m = o.material
            lines.append(f"object {o.type} " + num(list(o.position) + list(o.size) + [o.radius]) + f" {m.kind} "
                         + num(list(m.color) + [m.roughness, m.metallic, m.specular, m.refraction_index]))
        for i in range(v.num_lights):
            li = v.lights[i]
            lines.append("light " + num(list(li.position) + list(li.color) + [li.intensity]))
        lines.append("end")
    return "\n".join(lines) + "\n"


# ------------------------------------------------------------------ families
def _neg_zero_radius():
    """Radius -0.9 in metal, glass and lambertian (the outward normal flips,
    FrontFace inverts, S.r > 0 is false so the sphere never leaves itself out
    of its shadow cone, culling takes fabs(r)); a radius-0 sphere; a mirror
    behind them that sees their backs."""
    return scene([
        sph((-2.4, 0, 0), -0.9, METAL, {"radius": 0.9}),
        sph((-0.3, 0, 0.4), -0.9, GLASS, {"radius": 0.9}),
        sph((1.9, 0, 0), -0.9, RED, {"radius": 0.9}),
        sph((0.9, 1.4, 1.0), 0.0, GREEN, {"radius": 0.3}),
        sph((3.4, -0.5, 1.5), -0.5, ROUGH, {"radius": 0.5}),
        sph((0, 1.0, -3.2), 2.0, MIRROR),
    ])


def _coincident():
    """Exact duplicates with different materials (the last in hittable order
    wins every tie), two identical cubes, a sphere tangent to a cube face."""
    return scene([
        sph((-2.6, 0, 0), 0.8, METAL),
        sph((-2.6, 0, 0), 0.8, RED, None),
        sph((0, 0, 0.2), 0.8, GLASS),
        sph((0, 0, 0.2), 0.8, GLASS2, None),
        sph((0, 0, 0.2), 0.8, MIRROR, None),
        sph((2.6, 0, 0), 0.8, MIRROR),
        sph((2.6, 0, 0), 0.8, GREEN, None),
        cube((1.3, -0.6, 2.2), (0.7, 0.7, 0.7), METAL),
        cube((1.3, -0.6, 2.2), (0.7, 0.7, 0.7), BLUE, None),
        cube((-1.4, -0.6, 2.2), (0.8, 0.8, 0.8), LAMB),
        sph((-0.7, -0.6, 2.2), 0.3, ROUGH),  # touches the face x = -1.0
    ])


def _coincident_wide():
    """24 spheres and no cube (wide mode: closest_wide deals sphere i to helper
    i mod S, S = 16, 8 or 4).  The coincident partners' hittable indices differ
    by an odd number, so for every S they sit on different helpers and the tie
    is resolved by the cross-lane merge."""
    mats = [METAL, RED, GLASS, GREEN, ROUGH, MIRROR, BLUE, DIEL]
    objs = []
    for i in range(17):  # hittable indices 1..17 (the ground is 0)
        x = (i % 6) * 1.3 - 3.25
        z = -(i // 6) * 1.4 + 1.0
        objs.append(sph((x, -0.45 + 0.15 * (i % 3), z), 0.5, mats[i % 8]))
    # partners by hittable index: (5, 18), (2, 19), (9, 20) and 12 = 21 = 22 = 23 (23 wins over 22)
    for first, m in ((5, BLUE), (2, MIRROR), (9, RED), (12, GLASS2)):
        o = copy.deepcopy(objs[first - 1])
        objs.append(sph(o["position"], o["radius"], m, None))
    o = objs[12 - 1]
    objs.append(sph(o["position"], o["radius"], METAL, None))
    objs.append(sph(o["position"], o["radius"], GREEN, None))
    assert len(objs) == 23
    return scene(objs)


def _zero_neg_colour():
    """Colours with zero components (light_inert needs D without a zero
    component), black, and negative components; lights of intensity 0 and -10,
    a black light and lights with a zero colour component.  Negative radiance
    tone-maps to NaN and displays as byte 0."""
    return scene([
        sph((-3.0, 0, 0), 0.8, {"type": "lambertian", "color": [0, 0.7, 0.7]},
            {"material": {"type": "lambertian", "color": [0.3, 0.7, 0.7]}}),
        sph((-1.2, 0, 0.3), 0.8, {"type": "lambertian", "color": [0, 0, 0]}, {"material": LAMB}),
        sph((0.6, 0, 0), 0.8, {"type": "metal", "color": [0.9, 0, 0.5], "roughness": 0.2, "metallic": 0.6},
            {"material": METAL}),
        sph((2.4, 0, 0.3), 0.8, {"type": "lambertian", "color": [-0.5, 0.8, 0.3]}, {"material": GREEN}),
        sph((3.6, -0.4, 1.6), 0.5, {"type": "metal", "color": [0.8, -0.6, 0.4], "roughness": 0.0, "metallic": 1.0},
            {"material": MIRROR}),
        sph((-0.3, -0.6, 2.4), 0.4, {"type": "metal", "color": [0, 0, 0], "roughness": 0.3, "metallic": 0.2},
            {"material": ROUGH}),
        sph((0, 1.2, -3.0), 1.8, MIRROR),
    ], [
        light((0, 5, 2), (1, 0, 1), 15.0, None),
        light((2, 4, 3), (1, 1, 1), 0.0, None),
        light((-1.5, 0.6, 2.5), (1, 1, 1), -10.0, None),
        light((1, 3, 5), (0, 0, 0), 30.0, None),
        light((-3, 5, 1), (0, 1, 0), 10.0, None),
    ])


def _odd_materials():
    """One small sphere per out-of-range (finite) parameter set: the
    constructors' clamps (NewMetal's Min(x, 1.0) and its siblings) are part of
    what is rendered."""
    mats = [
        {"type": "metal", "color": [0.9, 0.7, 0.5], "roughness": 7.0, "metallic": -3.0, "specular": 9.0},
        {"type": "metal", "color": [0.8, 0.8, 0.9], "roughness": -0.5},
        {"type": "perfectmirror", "color": [0.9, 0.9, 0.8], "roughness": -2.0},
        {"type": "glass", "color": [0.9, 0.9, 1.0], "refractionIndex": 0.0},
        {"type": "glass", "color": [1.0, 0.9, 0.9], "refractionIndex": -1.5},
        {"type": "glass", "color": [0.9, 1.0, 0.9], "refractionIndex": 1.0},
        {"type": "dielectric", "refractionIndex": 1e300},
        {"type": "dielectric", "refractionIndex": 1e-300},
        {"type": "diffuselight", "color": [2.0, -1.0, 3.0]},
        {"type": "shiny", "color": [0.3, 0.6, 0.9], "roughness": -1.0, "metallic": 5.0, "specular": -2.0},
    ]
    fixes = [METAL, METAL, MIRROR, GLASS, GLASS, GLASS, DIEL, DIEL, {"type": "diffuselight", "color": [2, 1, 3]}, ROUGH]
    objs = []
    for i, (m, f) in enumerate(zip(mats, fixes)):
        x = (i % 5) * 1.5 - 3.0
        objs.append(sph((x, -0.4 if i < 5 else 1.0, 0.8 if i < 5 else -0.6), 0.6, m, {"material": f}))
    return scene(objs)


def _flat_cubes():
    """Cubes with zero and underflowing sizes: a zero size product leaves
    DBox.front_out "unknown" (-1), an underflowing one makes it 0; both give
    degenerate triangles (|a| < 1e-6) and zero-thickness slabs in ray_box."""
    return scene([
        cube((-2.4, 0.2, 0), (1.5, 0, 1.5), RED, {"size": [1.5, 0.4, 1.5]}),
        cube((0, 0.8, 0.5), (0, 0, 0), GREEN, {"size": [0.5, 0.5, 0.5]}),
        cube((0.2, 0, 0.5), (1.2, 1.2, 0), GLASS, {"size": [1.2, 1.2, 0.5]}),
        cube((2.6, 0.1, 0), (1, 1e-300, 1), METAL, {"size": [1, 0.4, 1]}),
        cube((-1.2, -0.6, 2.4), (0.7, 0.7, 0), BLUE, {"size": [0.7, 0.7, 0.3]}),
        sph((1.4, -0.5, 1.6), 0.5, ROUGH),
        sph((0, 1.0, -3.2), 2.0, MIRROR),
    ])


def _on_surfaces():
    """The camera at the centre of one glass sphere and exactly on the surface
    of another; a light at the camera, one 5e-4 above a surface (closer than
    the 0.001 at which a light is skipped), one exactly on a surface (light
    distance 0, the zero vector normalised) and one at a sphere's centre."""
    return scene([
        sph((0, 0.5, 6), 0.5, GLASS, None),                       # the camera is its centre
        sph((0, 0.5, 4.5), 1.5, DIEL, {"radius": 1.25}),          # the camera is on its surface
        sph((2.4, 0, 0), 0.9, LAMB),
        sph((-2.4, 0, 0), 0.9, RED),
        sph((0, 0, 0), 1.0, GLASS2),
        sph((0, 1.5, -3.5), 2.2, MIRROR),
    ], [
        light((0, 0.5, 6), (1, 0.9, 0.8), 3.0, None),
        light((2.4, 0.9005, 0), (1, 1, 1), 2.0, None),
        light((-2.4, 0.9, 0), (1, 1, 1), 2.0, None),
        light((0, 0, 0), (0.6, 0.8, 1), 4.0, None),
    ])


def _shell(p, r=0.35, m=None):
    """An opaque shell around a light: from outside its shadow rays are blocked."""
    return sph(p, r, m or LAMB)


def _nonfinite_lights():
    """Lights of intensity +Inf and 1e308, a NaN colour component, and position
    components of +Inf, NaN and 1e200 (the distance overflows).  The lights
    with a finite position sit inside opaque shells, so most of the frame is in
    their shadow and stays finite."""
    return scene([
        sph((-2.4, 0, 0), 0.9, METAL), sph((0, 0, 0.3), 0.9, GLASS), sph((2.4, 0, 0), 0.9, RED),
        sph((0, 1.2, -3.2), 2.0, MIRROR),
        _shell((-3.4, 1.6, 1.0)), _shell((3.4, 1.6, 1.0)), _shell((-1.2, 2.4, 0.5)),
        sph((1.2, -0.6, 2.4), 0.4, ROUGH),
    ], [
        light((-3.4, 1.6, 1.0), (1, 1, 1), INF, None),
        light((3.4, 1.6, 1.0), (1, 0.5, 0.2), 1e308, None),
        light((-1.2, 2.4, 0.5), (1, NAN, 1), 5.0, None),
        light((INF, 4, 2), (1, 1, 1), 30.0, None),
        light((1, NAN, 3), (1, 1, 1), 30.0, None),
        light((2, 1e200, 1), (1, 1, 1), 1e300, None),
    ])


def _material_row(mats):
    objs = [sph((-2.6, 0, 0), 0.9, METAL), sph((0, 0, 0), 0.9, GLASS), sph((2.6, 0, 0), 0.9, RED),
            sph((0, 1.4, -3.4), 2.0, MIRROR)]
    for i, (m, f) in enumerate(mats):
        objs.append(sph((i * 1.3 - 3.25, -0.65, 2.2), 0.35, m, {"material": f}))
    return scene(objs)


def _nonfinite_materials():
    """Roughness NaN, refractionIndex NaN and Inf, metallic Inf, a diffuselight
    of colour (-1, NaN, Inf): NaN directions and NaN radiance flow down the
    paths that meet them."""
    return _material_row([
        ({"type": "metal", "color": [0.9, 0.8, 0.7], "roughness": NAN, "metallic": 0.9}, METAL),
        ({"type": "glass", "color": [0.9, 0.95, 1.0], "refractionIndex": NAN}, GLASS),
        ({"type": "dielectric", "refractionIndex": INF}, DIEL),
        ({"type": "metal", "color": [0.9, 0.6, 0.3], "roughness": 0.2, "metallic": INF}, ROUGH),
        ({"type": "diffuselight", "color": [-1.0, NAN, INF]}, {"type": "diffuselight", "color": [1, 2, 3]}),
    ])


def _nonfinite_materials_inf_colour():
    """A colour component of +Inf: the attenuation of every path that scatters
    here is infinite in that channel, and what it multiplies decides between
    Inf and NaN (the reference multiplies the black of a miss: Inf * 0)."""
    return _material_row([
        ({"type": "lambertian", "color": [0.5, INF, 0.5]}, LAMB),
        ({"type": "metal", "color": [INF, 0.8, 0.7], "roughness": 0.1, "metallic": 0.3}, METAL),
    ])


def _geometry_base():
    return [sph((-2.4, 0, 0), 0.9, METAL), sph((0, 0, 0.3), 0.9, GLASS), sph((2.4, 0, 0), 0.9, RED),
            sph((0, 1.2, -3.2), 2.0, MIRROR), cube((1.3, -0.6, 2.2), (0.7, 0.7, 0.7), BLUE)]


def _nonfinite_geometry():
    """One non-finite object per scene (a NaN sphere or cube is hit by every
    ray at t = NaN, so the whole image is NaN; an Inf-radius sphere swallows
    the frame), and one scene with the NaN objects first in hittable order,
    where later hittables still replace them."""
    out = {}
    one = {
        "nan_radius": sph((1, 0.5, 1), NAN, GREEN, None),
        "nan_centre": sph((1, NAN, 1), 0.5, GREEN, None),
        "inf_radius": sph((0, 0, -50), INF, GREEN, None),
        "inf_centre": sph((INF, 0.5, 1), 0.5, GREEN, None),
        "nan_cube": cube((1, 0.5, 1), (0.5, NAN, 0.5), GREEN, None),
        "inf_cube": cube((1, 0.5, 1), (0.5, INF, 0.5), GREEN, None),
    }
    for name, o in one.items():
        out["nonfinite_geometry_" + name] = scene(_geometry_base() + [o])
    first = {"camera": copy.deepcopy(CAM),
             "objects": [sph((1, 0.5, 1), NAN, GREEN, None), sph((1, NAN, 1), 0.5, ROUGH, None),
                         cube((-1, 0.5, 1), (0.5, NAN, 0.5), GREEN, None), copy.deepcopy(GROUND)] + _geometry_base(),
             "lights": copy.deepcopy(LIGHTS)}
    out["nonfinite_geometry_nan_first"] = first
    return out


def _field(sc):
    """The scene laid over a field of 72 finite small spheres (more than 64:
    the BVH and wavefront path by default); cubes are dropped (the BVH is over
    spheres)."""
    out = spheres_only(sc)
    mats = [METAL, GLASS, RED, DIEL]
    for i in range(72):
        x = (i % 12) * 0.62 - 3.41
        z = -(i // 12) * 0.7 + 3.4
        out["objects"].append(sph((x, -0.8 + 0.1 * (i % 3), z), 0.2, mats[i % 4]))
    return out


def _families():
    fam = {
        "neg_zero_radius": _neg_zero_radius(),
        "coincident": _coincident(),
        "coincident_wide": _coincident_wide(),
        "zero_neg_colour": _zero_neg_colour(),
        "odd_materials": _odd_materials(),
        "flat_cubes": _flat_cubes(),
        "on_surfaces": _on_surfaces(),
        "nonfinite_lights": _nonfinite_lights(),
        "nonfinite_materials": _nonfinite_materials(),
        "nonfinite_materials_inf_colour": _nonfinite_materials_inf_colour(),
    }
    fam.update(_nonfinite_geometry())
    for name in ("odd_materials", "nonfinite_materials", "nonfinite_materials_inf_colour", "nonfinite_lights",
                 "neg_zero_radius", "coincident"):
        fam["field70_" + name] = _field(fam[name])
    return fam


SCENES = _families()

FINITE = [n for n, s in SCENES.items() if is_finite(s)]
GEOMETRY = [n for n in SCENES if n.startswith("nonfinite_geometry_")]
FIELD = [n for n in SCENES if n.startswith("field70_")]
LINEAR = [n for n in SCENES if n not in FIELD]  # at most 64 spheres and 64 triangles
# families meant to produce special values: NaN / Inf radiance, or negative
# radiance (NaN after the tone map, byte 0)
SPECIAL = ["zero_neg_colour", "nonfinite_lights", "nonfinite_materials", "nonfinite_materials_inf_colour",
           "field70_nonfinite_lights", "field70_nonfinite_materials", "field70_nonfinite_materials_inf_colour"]

for _n in LINEAR:
    _o = SCENES[_n]["objects"]
    assert sum(o["type"] == "sphere" for o in _o) <= 64 and 12 * sum(o["type"] == "cube" for o in _o) <= 64, _n
for _n in FIELD:
    assert sum(o["type"] == "sphere" for o in SCENES[_n]["objects"]) > 70 + 1, _n
