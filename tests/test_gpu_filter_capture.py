"""The denoise mode's capture (setting "filter"; shade_path's FILT variant): the two accumulator planes and the
features / worldPos records of each pixel's first non-specular vertex.

Bars: plane 0 + plane 1 equals the filter-off accumulator of the same frame, rgb and depth (w), within rel-L2 1e-4 (the
project's frame bar: only the order of the atomic additions differs); the ray counts are identical; for primary hits on
plain diffuse and on emissive materials features.z is the t of trace_closest on the frame's eye rays (aperture 0),
worldPos is O + t D, the material id and the 10:11:11 albedo are the hit material's; misses carry the sentinel record; behind
a mirror the specular flag is set and the records describe the vertex the reflected ray finds."""
import numpy as np
import pytest

import filter_ref as R
from lighthouse2_amd import abi, scene

pytestmark = pytest.mark.gpu

W, H = 128, 72


def _r0():
    s = 0x12345678
    s ^= (s << 13) & 0xffffffff
    s ^= s >> 17
    s ^= (s << 5) & 0xffffffff
    return s


def _frame_pair(core, sc):
    """The same frame with the filter off and on."""
    sc.load_into(core)
    core.set_target(W, H, 1)
    core.setting("filter", 0)
    sc.render_frame(core)
    off = dict(acc=core.accumulator(), counts=core.ray_counts())
    core.setting("filter", 1)
    sc.render_frame(core)
    on = dict(counts=core.ray_counts(), acc=core.filter_buffer("acc"), features=core.filter_buffer("features"),
              worldPos=core.filter_buffer("worldPos"), deltaDepth=core.filter_buffer("deltaDepth"))
    o, d, _ = core.generate_eye_rays(sc.view, _r0(), 0)
    hits = core.trace_closest(o, d)
    core.setting("filter", 0)
    return off, on, o, d, hits


def _half(c):
    return np.asarray(c, np.float16).astype(np.float32)


def _material_table(sc):
    """Per material: plain diffuse (no map, no cut-out, rough, opaque, not emissive), emissive, mapped diffuse (colour or normal
    maps, but no cut-out and no roughness map: its albedo is not the material's colour alone), and its colour."""
    rows = []
    for m in sc.materials:
        col = np.array([m.color.value.x, m.color.value.y, m.color.value.z], np.float32)
        mapped = any(getattr(m, f).textureID >= 0 for f in ("color", "detailColor", "normals", "detailNormals", "roughness"))
        emissive = bool((col > 1).any())
        diffuse = not (m.flags & 2) and m.roughness.value > 0.01 and m.transmission.value < 0.5 and not emissive
        rows.append((diffuse and not mapped, emissive and not mapped, col, diffuse and mapped and m.roughness.textureID < 0))
    return rows


@pytest.mark.parametrize("name,make", [
    ("room", lambda: scene.room_scene(20000, W, H)),
    ("config2_light", lambda: scene.config2_scene(n=5000, width=W, height=H, sky=True, light=True)),
    ("textured", lambda: scene.textured_scene(W, H, tess=8))])
def test_capture_matches_unfiltered_frame(fresh_core, name, make):
    sc = make()
    off, on, o, d, hits = _frame_pair(fresh_core, sc)
    # the planes
    total = on["acc"][0] + on["acc"][1]
    ref = off["acc"]
    rel = float(np.linalg.norm(total[..., :3] - ref[..., :3]) / np.linalg.norm(ref[..., :3]))
    rel_w = float(np.linalg.norm(total[..., 3] - ref[..., 3]) / np.linalg.norm(ref[..., 3]))
    print(f"{name}: planes vs accumulator rel-L2 rgb {rel:.2e} w {rel_w:.2e}; indirect share "
          f"{np.abs(on['acc'][1][..., :3]).sum() / max(np.abs(total[..., :3]).sum(), 1e-30):.3f}")
    assert rel <= 1e-4 and rel_w <= 1e-4, (rel, rel_w)
    assert np.array_equal(on["acc"][1][..., 3], np.zeros((H, W), np.float32))   # the depth is a first-vertex quantity
    assert np.array_equal(off["counts"], on["counts"]), (off["counts"], on["counts"])
    # the records of the primary hits
    feat = on["features"].reshape(-1, 4)
    wpos = on["worldPos"].reshape(-1, 4)
    t = hits[:, 0].view(np.float32)
    prim = hits[:, 1].view(np.int32)
    inst = hits[:, 2].view(np.int32)
    hit = prim != -1
    mesh_of = np.array([m for m, _ in sc.instances], np.int64)
    mat = np.zeros(len(prim), np.int64)
    for mi, tris in enumerate(sc.meshes):
        sel = hit & (mesh_of[np.where(hit, inst, 0)] == mi)
        mat[sel] = tris.view(np.uint32)[prim[sel], abi.TRI["material"]]
    table = _material_table(sc)
    plain = hit & np.array([table[m][0] for m in mat])
    emissive = hit & np.array([table[m][1] for m in mat])
    textured = hit & np.array([table[m][3] for m in mat])
    print(f"{name}: {int(plain.sum())} plain diffuse, {int(textured.sum())} mapped diffuse, {int(emissive.sum())} emissive, "
          f"{int((~hit).sum())} missed of {len(hit)} pixels")
    assert (plain | textured).sum() > 100
    for sel, what in ((plain, "diffuse"), (emissive, "emissive"), (textured, "mapped")):
        if not sel.any():
            continue
        assert np.array_equal(feat[sel, 2].view(np.float32), t[sel]), what
        p = (o[sel, :3] + t[sel, None] * d[sel, :3]).astype(np.float32)
        assert np.array_equal(wpos[sel, :3], p), what
        assert np.array_equal(feat[sel, 3] >> 6, mat[sel].astype(np.uint32)), what
        assert np.array_equal((feat[sel, 3] >> 4) & 3, np.zeros(int(sel.sum()), np.uint32)), what
        assert np.array_equal(feat[sel, 3] & 15, np.zeros(int(sel.sum()), np.uint32)), what   # first frame: no history
        if what != "mapped":
            colour = np.stack([_half(table[m][2]) for m in mat[sel]])
            assert np.array_equal(feat[sel, 0], R.pack_rgb(colour)), what
        assert np.array_equal(wpos[sel, 3].view(np.uint32), feat[sel, 1]), what               # the packed normal twice
    # the depth derivatives of a diffuse hit are finite (but for a grazing plane), and zero for the sentinel
    dd = on["deltaDepth"].reshape(-1, 4)
    assert np.isfinite(dd[plain | textured]).mean() > 0.99 and np.array_equal(dd[:, :2], np.zeros((len(dd), 2), np.float32))
    # misses: the sentinel
    miss = ~hit
    if miss.any():
        assert np.array_equal(feat[miss, 2].view(np.float32), np.full(int(miss.sum()), R.MISS_T, np.float32))
        assert np.array_equal(feat[miss, 3] >> 4, np.zeros(int(miss.sum()), np.uint32))
        far = (o[miss, :3] + np.float32(50000.0) * d[miss, :3]).astype(np.float32)
        assert np.array_equal(wpos[miss, :3], far)
        assert np.array_equal(feat[miss, 1], R.pack_normal(-d[miss, :3]))
        assert np.array_equal(dd[miss], np.zeros((int(miss.sum()), 4), np.float32))


def _mirror_scene():
    """A red floor, a mirror wall facing the camera (metallic 1, roughness 0: the BSDF's specular lobe alone, at its narrowest,
    GGX alpha 0.001), a light above: the mirror's pixels see the floor and the sky."""
    mats = [abi.make_material((0.7, 0.2, 0.1), roughness=1.0),     # 0 floor
            abi.make_material((0.9, 0.8, 0.6), roughness=0.0, metallic=1.0),   # 1 mirror
            abi.make_material((20.0, 20.0, 20.0))]                 # 2 light
    floor = scene.quad_tris((0, 1, 0), (0, 0, 0), 30, 30, 0)
    mirror = scene.quad_tris((0, 0, -1), (0, 2, 4), 6, 4, 1)
    light = scene.quad_tris((0, -1, 0), (0, 9, 0), 3, 3, 2)
    light.view(np.int32)[:, abi.TRI["ltriIdx"]] = [0, 1]
    tris = np.concatenate([floor, mirror, light]).astype(np.float32)
    sc = scene.Scene(meshes=[tris], instances=[(0, np.eye(4, dtype=np.float32))], materials=mats, name="mirror")
    sc.area_lights = [scene.light_from_tri(tris[4 + i], 4 + i, 0, (20.0, 20.0, 20.0)) for i in range(2)]
    sc.sky = scene.gradient_sky(64, 32)
    sc.view = scene.camera_view((0, 2.5, -6), (0, -0.1, 1), fov_deg=50, aspect=W / H, focal=5, pixel_height=H)
    return sc


def test_capture_behind_a_mirror(fresh_core):
    sc = _mirror_scene()
    off, on, o, d, hits = _frame_pair(fresh_core, sc)
    total = on["acc"][0] + on["acc"][1]
    rel = float(np.linalg.norm(total[..., :3] - off["acc"][..., :3]) / np.linalg.norm(off["acc"][..., :3]))
    assert rel <= 1e-4, rel
    assert np.array_equal(off["counts"], on["counts"])
    feat = on["features"].reshape(-1, 4)
    wpos = on["worldPos"].reshape(-1, 4)
    t = hits[:, 0].view(np.float32)
    prim = hits[:, 1].view(np.int32)
    on_mirror = (prim == 2) | (prim == 3)
    assert on_mirror.sum() > 200
    # via a specular vertex (but for the few paths the lobe's tail sends under the mirror: they end there, the sentinel stays)
    via = ((feat[:, 3] >> 4) & 3) == 1
    assert via[on_mirror].mean() > 0.98 and not via[~on_mirror].any()
    sel = on_mirror & via
    assert np.array_equal(feat[sel, 1] & 3, np.ones(int(sel.sum()), np.uint32))
    assert np.array_equal(wpos[sel, 3].view(np.uint32), feat[sel, 1])
    # the ideal reflected rays, traced from the mirror's plane
    I = o[sel, :3] + t[sel, None] * d[sel, :3]
    n = np.array([0, 0, -1], np.float32)
    Rd = d[sel, :3] - 2 * (d[sel, :3] @ n)[:, None] * n
    ro = np.concatenate([I + 1e-3 * n, np.zeros((len(I), 1), np.float32)], 1).astype(np.float32)
    rd = np.concatenate([Rd, np.full((len(I), 1), 1e34, np.float32)], 1).astype(np.float32)
    h2 = fresh_core.trace_closest(ro, rd)
    t2, prim2 = h2[:, 0].view(np.float32), h2[:, 1].view(np.int32)
    f, p = feat[sel], wpos[sel]
    on_floor = (f[:, 2].view(np.float32) < 1e30) & ((f[:, 3] >> 6) == 0)     # the record says: the floor
    ideal_floor = (prim2 == 0) | (prim2 == 1)
    assert on_floor.sum() > 50 and (~on_floor).sum() > 50
    assert (on_floor == ideal_floor).mean() > 0.97
    # the recorded vertex lies on the floor, features.z is its distance from the mirror, and it is where the ideal mirror puts it
    # up to the lobe's width (alpha 0.001: the bulk within a few mrad, so the median pixel within 0.05 at these distances)
    assert np.abs(p[on_floor, 1]).max() <= 1e-3
    dist = np.linalg.norm(p[on_floor, :3] - I[on_floor], axis=1)
    assert np.allclose(f[on_floor, 2].view(np.float32), dist, rtol=1e-3, atol=1e-3)
    both = on_floor & ideal_floor
    off_ideal = np.linalg.norm(p[both, :3] - (ro[both, :3] + t2[both, None] * rd[both, :3]), axis=1)
    print(f"mirror: {int(sel.sum())} pixels, {int(on_floor.sum())} see the floor; distance from the ideal reflection: median "
          f"{np.median(off_ideal):.4f}, max {off_ideal.max():.3f}")
    assert np.median(off_ideal) <= 0.05
    # albedo: the floor's colour times the mirror's (as 10:11:11 stored it at the specular vertex)
    mirror_c = R.unpack_rgb(R.pack_rgb(_half([0.9, 0.8, 0.6])), np.float32)
    assert np.array_equal(f[on_floor, 0], np.full(int(on_floor.sum()), R.pack_rgb(_half([0.7, 0.2, 0.1]) * mirror_c), np.uint32))
    sky = f[:, 2].view(np.float32) > 1e30
    assert sky.sum() > 50 and np.array_equal(f[sky, 3] >> 6, np.zeros(int(sky.sum()), np.uint32))
