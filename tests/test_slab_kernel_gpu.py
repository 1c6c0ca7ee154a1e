"""render_slab7_kernel: the pair kernels' walk with cuboid_slab in cuboid_range's place (rtgo_device.h).  A certified
cuboid that also holds the build's slab certificate is, in the frame of its first face, an axis-aligned box; a slab test on the hardware
reciprocal says which one face the ray can meet, and that face alone gets the reference's test (rect_commit: the same operations on the
same values).  The steering arithmetic must never leave out a face the reference accepts, so everything a launch leaves -- every pixel
of the accumulation buffer, the 8-bit image, the ray count -- must be what the same launch leaves with RTGO_NO_SLAB=1 (render_pair7_kernel)
and what the canonical walk leaves (a collect_stats launch), bit for bit; rtgo_stats.last_variant bit 10 says the slab kernel ran.

Then the certificate itself, read back through rtgo_debug_read_build (Context.read_build): where it holds its numbers are checked
against float64 from the model matrices, and the scenes it must refuse render with bit 10 clear.
RTGO_MAX_WPE=7 pins the seven-waves kernels on these small frames, RTGO_TREE=0 the first fast-walk structure.  Needs a real MI355X."""
import numpy as np
import pytest

import adversarial_cameras as A
from test_lane_mask_votes_gpu import INSIDE, face_frame, in_room
from test_pair_walk import BOX_A, BOX_B, FULL, POSE_A, POSE_B, ROOM, Env, reposed, seeded_scene, tables, trs

pytestmark = pytest.mark.gpu

PAIR, PAIR7, SLAB, CANON = 256, 512, 1024, 4
CUBOID_TOL = 1e-4   # kCuboidTol (rtgo_device.h)


def render(t, W, H, N, frames, cam=None, max_depth=5, bands=FULL, window=None, stats=False, env=None, build=False):
    """accum and image of the launch's rows after `frames` progressive frames, rays_total, last_variant of every launch (and the build)"""
    from raytracingo_amd import capi
    kv = {"RTGO_MAX_WPE": "7", "RTGO_TREE": "0", "RTGO_NO_SLAB": None, "RTGO_NO_PAIR": None}
    kv.update(env or {})
    with Env(**kv):
        ctx = capi.Context(0)
        try:
            ctx.set_scene(t["type"], t["M"], t["mat"], t["aabb"])
            c = t["cam"] if cam is None else cam
            ctx.set_camera(c[0:3], c[3:6], c[6:9], c[9:12])
            ctx.set_background(t["bg"])
            ctx.set_lights(t["lights"])
            x0, y0, w, h = window if window else (0, 0, W, H)
            rows = capi.local_rows(h, *bands)
            ctx.resize(rows * w)
            variants = []
            for f in range(frames):
                ctx.launch(capi.make_frame(W, H, N, f, True, max_depth=max_depth, bands=bands, window=window, stats=stats))
                ctx.sync()
                variants.append(ctx.stats()["last_variant"])
            out = (ctx.read_accum(rows, w).copy(), ctx.read_image(rows, w).copy(), ctx.stats()["rays_total"], variants)
            return out + ((ctx.read_build(False),) if build else ())
        finally:
            ctx.close()


def three_walks(t, W, H, N, frames, slab=True, pair=True, **kw):
    """the job on the slab kernel, on the pair kernel (RTGO_NO_SLAB=1) and on the canonical walk: the same bits in every pixel, the same
    image, the same rays.  slab / pair: whether the first two are expected to take those kernels.  Returns the variants of the first."""
    a_s, i_s, r_s, v_s = render(t, W, H, N, frames, **kw)
    a_p, i_p, r_p, v_p = render(t, W, H, N, frames, env={"RTGO_NO_SLAB": "1"}, **kw)
    a_c, i_c, r_c, v_c = render(t, W, H, N, frames, stats=True, **kw)
    assert all(bool(v & SLAB) == slab for v in v_s), v_s
    assert all(not (v & SLAB) or (v & PAIR and v & PAIR7) for v in v_s), v_s
    assert all(not v & SLAB and bool(v & PAIR) == pair for v in v_p), v_p
    assert all(v & CANON and not v & (PAIR | SLAB) for v in v_c), v_c
    assert r_s == r_p == r_c, (r_s, r_p, r_c)
    for name, a, i in (("pair kernel", a_p, i_p), ("canonical walk", a_c, i_c)):
        assert a_s.tobytes() == a.tobytes(), "slab kernel != %s: %d pixels" % (name, int(np.sum(np.any(a_s != a, axis=-1))))
        assert i_s.tobytes() == i.tobytes(), name
    return v_s


# ---- cornell

@pytest.mark.parametrize("max_depth", [0, 1, 5])
@pytest.mark.parametrize("sample", [2, 4])
def test_cornell_frames_0_to_2(sample, max_depth):
    three_walks(tables("cornell", 160, 90), 160, 90, sample, 3, max_depth=max_depth)


def test_cornell_window():
    three_walks(tables("cornell", 160, 90), 160, 90, 2, 2, window=(48, 20, 70, 37))


def test_cornell_one_of_three_band_shares():
    three_walks(tables("cornell", 160, 90), 160, 90, 2, 2, bands=(4, 3, 1))


def test_debug_line_names_the_slab_kernel(capfd):
    t = tables("cornell", 96, 64)
    capfd.readouterr()
    *_, v = render(t, 96, 64, 2, 1, env={"RTGO_DEBUG": "1"})
    err = capfd.readouterr().err
    lines = [l for l in err.splitlines() if l.startswith("rtgo_launch:")]
    assert len(lines) == 1 and " kernel render_slab7_kernel," in lines[0], err[-2000:]
    assert all(x & SLAB for x in v), v
    scene = [l for l in err.splitlines() if l.startswith("rtgo_set_scene:")]
    assert len(scene) == 1 and "slab certificate 1)" in scene[0] and "two-leaf tree: 1 1)" in scene[0], scene


# ---- adversarial cameras, 64 x 64

W = H = 64


@pytest.mark.parametrize("axis,c,eye_ab,w_ab,_", A.CORNELL_PLANES, ids=["%s=%g" % ("xyz"[p[0]], p[1]) for p in A.CORNELL_PLANES])
def test_camera_in_an_axis_aligned_face_plane(axis, c, eye_ab, w_ab, _):
    # the six walls, the boxes' bottoms and tops, the lamp
    cam = A.in_plane(axis, c, eye_ab, w_ab)
    assert A.zero_axes(cam) == [axis]
    three_walks(tables("cornell", W, H), W, H, 2, 1, cam=cam)


def in_face_plane(t, row):
    """a camera in the plane of rectangle `row`, beyond one of its edges, whose U, V and W lie in that plane"""
    c, ex, ez, _ = face_frame(t, row)
    ux, uz = ex / np.linalg.norm(ex), ez / np.linalg.norm(ez)
    for s in (1.0, -1.0):
        eye = c + s * (0.5 * ex + 0.6 * ux)
        if bool(np.all(np.abs(eye) <= 4.0 + 1e-6)):   # (the boxes' bottoms lie in the floor's plane: the room's closed box)
            cam = np.zeros(12, np.float32)
            cam[0:3], cam[3:6], cam[6:9], cam[9:12] = eye, uz, ux, -s * (0.8 * ux) + 0.15 * uz
            return cam
    raise AssertionError("no eye inside the room for face %d" % row)


@pytest.mark.parametrize("row", list(range(BOX_A.start, BOX_A.stop)) + list(range(BOX_B.start, BOX_B.stop)))
def test_camera_in_the_plane_of_a_box_face(row):
    t = tables("cornell", W, H)
    three_walks(t, W, H, 2, 1, cam=in_face_plane(t, row))


@pytest.mark.parametrize("box", [BOX_A, BOX_B], ids=["short", "tall"])
def test_one_ray_along_a_box_edge(box):
    t = tables("cornell", W, H)
    c, ex, ez, _ = face_frame(t, box.start)
    along = ex / np.linalg.norm(ex)
    eyes = [(c + s * 0.5 * ex + 0.5 * ez + s * along, -s * along) for s in (1.0, -1.0)]
    eye, d = next((e, d) for e, d in eyes if in_room(e))
    three_walks(t, W, H, 2, 1, cam=A.one_ray(eye.astype(np.float32), d.astype(np.float32)))


@pytest.mark.parametrize("corner", [(-4.0, -4.0, -4.0), (4.0, 4.0, -4.0)])
def test_one_ray_through_a_room_corner(corner):
    d = np.array(corner) - INSIDE.astype(np.float64)
    three_walks(tables("cornell", W, H), W, H, 2, 1, cam=A.one_ray(INSIDE, d.astype(np.float32)))


def test_one_ray_through_a_box_corner():
    t = tables("cornell", W, H)
    c, ex, ez, _ = face_frame(t, BOX_A.start)
    corner = c + 0.5 * ex + 0.5 * ez
    d = corner - INSIDE.astype(np.float64)
    three_walks(t, W, H, 2, 1, cam=A.one_ray(INSIDE, d.astype(np.float32)))


def list_frame_rows(build):
    """rows 0..2 of the first record of the up-front list of tree 0, the frame of the room's slab certificate, and its parallel threshold"""
    meta = np.ascontiguousarray(build["tree0.meta"]).view(np.int32)
    fp = np.asarray(build["tree0.fprims"], np.float32).reshape(-1, 4, 4)
    first = int(meta[2])
    return fp[first, 0:3, 0:3], float(fp[first + 4, 3, 2])


@pytest.mark.parametrize("axis,c,eye_ab", [(0, -4.0, (-3.3, -0.7)), (2, 4.0, (-0.7, -3.3))], ids=["x=-4", "z=4"])
def test_every_primary_takes_the_flat_ray_fall_back(axis, c, eye_ab):
    # W exactly along a wall: U, V and W are exactly 0 on `axis`, so every primary's direction is; one row of the room's frame is that
    # axis up to the residues of the matrix's own rounding (4e-8), so |d_a| of that row is far below the certificate's threshold for
    # every primary (float64 here; half the threshold leaves the kernel's float32 all the room it needs): the six single tests run for
    # every primary ray of the frame (and for whichever bounce rays come as close)
    t = tables("cornell", W, H)
    cam = A.in_plane(axis, c, eye_ab)
    _, d, _ = A.rays(cam, W, H, 0)
    assert (d[:, axis] == 0).all()
    *_, v, build = render(t, W, H, 2, 1, cam=cam, build=True)
    assert all(x & SLAB for x in v), v
    R, thr = list_frame_rows(build)
    da = np.abs(d.astype(np.float64) @ R.astype(np.float64).T)      # [ray, frame axis]
    assert thr > 0 and any((da[:, k] <= 0.5 * thr).all() for k in range(3)), (R, thr, da.max(axis=0))
    three_walks(t, W, H, 2, 1, cam=cam)


# ---- the certificate

def certificates(build):
    """(the list holds the slab certificate, the two leaves' bits) of tree 0, as the decoded meta reports them, checked against the packed
    fields they come from"""
    dec = np.ascontiguousarray(build["tree0.decoded"]).view(np.int32)
    slab_list, slab_leaves = int(dec[-2]), int(dec[-1])
    meta = np.ascontiguousarray(build["tree0.meta"]).view(np.int32)
    assert bool((int(meta[9]) >> 8) & 4) == bool(slab_list)
    fn = np.asarray(build["tree0.fnodes"], np.float32).reshape(-1, 2, 4)
    if len(fn) == 3:
        links = [-int(fn[k, 1, 3:4].view(np.int32)[0]) for k in (1, 2)]
        assert [bool((l >> 20) & 4) for l in links] == [bool(slab_leaves & 1), bool(slab_leaves & 2)]
    return slab_list, slab_leaves


def check_numbers(build, t, first):
    """the slab certificate's numbers of the group at records [first, first + 6) against float64 from the model matrices"""
    fp = np.asarray(build["tree0.fprims"], np.float32).reshape(-1, 4, 4)
    orig = fp[first:first + 6, 3, 1].copy().view(np.int32)
    M = t["M"][orig].astype(np.float64).reshape(6, 4, 4)
    F = np.linalg.inv(M[0])                           # the frame: the first face's object space
    sq = np.array([[x, 0.0, z, 1.0] for x in (-0.5, 0.5) for z in (-0.5, 0.5)])
    corners = np.einsum("ij,fjk,ck->fci", F, M, sq)[:, :, :3]      # [face, corner, axis]
    lo, hi = corners.min(axis=(0, 1)), corners.max(axis=(0, 1))
    got_lo, got_hi = fp[first:first + 3, 3, 2].astype(np.float64), fp[first:first + 3, 3, 3].astype(np.float64)
    assert np.all(np.abs(got_lo - lo) <= 2 * CUBOID_TOL) and np.all(np.abs(got_hi - hi) <= 2 * CUBOID_TOL), (got_lo, lo, got_hi, hi)
    assert np.all(got_hi > got_lo)
    map_ = int(fp[first + 3, 3, 2:3].view(np.int32)[0])
    faces = [(map_ >> (3 * s)) & 7 for s in range(6)]
    assert sorted(faces) == list(range(6)), faces
    for s, f in enumerate(faces):                     # plane s = 2 * axis + side holds face f: its corners lie on that plane
        bound = (hi if s & 1 else lo)[s >> 1]
        assert np.all(np.abs(corners[f, :, s >> 1] - bound) <= 2 * CUBOID_TOL), (s, f)
    rho, thr = float(fp[first + 3, 3, 3]), float(fp[first + 4, 3, 2])
    assert 1.0 <= rho < 1e6 and thr > 0.0
    assert abs(thr - 2e-5 * np.abs(F[:3, :3]).sum(axis=1).max()) <= 1e-3 * thr


def built(t):
    *_, v, build = render(t, 32, 32, 1, 1, build=True)
    return v, build


def test_certificate_holds_for_cornell():
    t = tables("cornell", 32, 32)
    v, build = built(t)
    assert certificates(build) == (1, 3)
    meta = np.ascontiguousarray(build["tree0.meta"]).view(np.int32)
    fn = np.asarray(build["tree0.fnodes"], np.float32).reshape(-1, 2, 4)
    for first in (int(meta[2]), int(fn[1, 0, 3:4].view(np.int32)[0]), int(fn[2, 0, 3:4].view(np.int32)[0])):
        check_numbers(build, t, first)
    assert all(x & SLAB for x in v)


def test_certificate_holds_for_boxes_turned_and_scaled():
    t, cam = seeded_scene(1, 32, 32)       # both boxes in the air at random rotations and scales
    v, build = built(t)
    assert certificates(build) == (1, 3)
    fn = np.asarray(build["tree0.fnodes"], np.float32).reshape(-1, 2, 4)
    for k in (1, 2):
        check_numbers(build, t, int(fn[k, 0, 3:4].view(np.int32)[0]))
    three_walks(t, W, H, 2, 1, cam=cam)


def copy_of(t):
    return {k: x.copy() for k, x in t.items()}


def sheared(t):
    S = np.eye(4)
    S[0, 1] = 0.2        # x += 0.2 y: a parallelepiped
    reposed(t, BOX_A, POSE_A, POSE_A @ S)
    return t


def face_moved(t):
    # one face of the short box moved outwards along its normal by 1e-3 of the box's size
    row = BOX_A.start
    M = t["M"][row].astype(np.float64).reshape(4, 4)
    n = M[:3, 1] / np.linalg.norm(M[:3, 1])
    M[:3, 3] += 1e-3 * 2.0 * n
    t["M"][row] = M.astype(np.float32).reshape(16)
    t["aabb"][row, 0:3] -= np.float32(4e-3)
    t["aabb"][row, 3:6] += np.float32(4e-3)
    return t


def wall_tilted(t):
    # one wall of the room turned by 1e-4 rad about an axis in its own plane, through its centre
    row = ROOM.start
    M = t["M"][row].astype(np.float64).reshape(4, 4)
    axis = M[:3, 0] / np.linalg.norm(M[:3, 0])
    T = trs([0, 0, 0], axis, 1e-4, [1, 1, 1])
    c = M[:3, 3].copy()
    M2 = M.copy()
    M2[:3, :3] = T[:3, :3] @ M[:3, :3]
    M2[:3, 3] = c
    t["M"][row] = M2.astype(np.float32).reshape(16)
    t["aabb"][row, 0:3] -= np.float32(4e-3)
    t["aabb"][row, 3:6] += np.float32(4e-3)
    return t


def far_cube(t):
    # the short box as a unit cube 1e4 units from the origin: its margin, K (cub_b ~ 1e4), is beyond what any launch accepts
    reposed(t, BOX_A, POSE_A, trs([1e4, 0.0, 0.0], [0, 1, 0], 0.3, [1.0, 1.0, 1.0]))
    return t


REFUSED = {"box face moved by 1e-3": (face_moved, 1), "wall tilted by 1e-4 rad": (wall_tilted, 0), "cube at 1e4": (far_cube, 1)}


@pytest.mark.parametrize("what", list(REFUSED))
def test_certificate_is_refused_and_the_slab_kernel_not_taken(what):
    make, which = REFUSED[what]
    t = make(copy_of(tables("cornell", W, H)))
    _, build = built(t)
    slab_list, slab_leaves = certificates(build)
    held = [slab_list] + [slab_leaves & 1, slab_leaves & 2]
    # (which group is the changed one: 0 the room; the boxes by their records' SBT rows)
    if which == 0:
        assert not slab_list, held
    else:
        fn = np.asarray(build["tree0.fnodes"], np.float32).reshape(-1, 2, 4)
        fp = np.asarray(build["tree0.fprims"], np.float32).reshape(-1, 4, 4)
        if len(fn) == 3:
            for k in (1, 2):
                first = int(fn[k, 0, 3:4].view(np.int32)[0])
                rows = set(fp[first:first + 6, 3, 1].copy().view(np.int32).tolist())
                if rows == set(range(BOX_A.start, BOX_A.stop)):
                    assert not slab_leaves & (1 << (k - 1)), held
        assert slab_leaves != 3, held
    a_s, i_s, r_s, v_s = render(t, W, H, 2, 1)
    a_c, i_c, r_c, v_c = render(t, W, H, 2, 1, stats=True)
    assert not any(x & SLAB for x in v_s), v_s
    assert all(x & CANON for x in v_c), v_c
    assert r_s == r_c
    assert a_s.tobytes() == a_c.tobytes(), "%s: %d pixels differ from the canonical walk" % (what, int(np.sum(np.any(a_s != a_c, axis=-1))))
    assert i_s.tobytes() == i_c.tobytes()


def test_certificate_holds_for_a_box_sheared_as_a_whole():
    # the frame is the first face's object frame, an affine one: with every face's matrix under the same shear the six faces are an
    # axis-aligned box in it, the normals' covectors stay parallel to its axes, and the slab test in affine coordinates is the same test
    t = sheared(copy_of(tables("cornell", W, H)))
    v, build = built(t)
    assert certificates(build) == (1, 3)
    fn = np.asarray(build["tree0.fnodes"], np.float32).reshape(-1, 2, 4)
    for k in (1, 2):
        check_numbers(build, t, int(fn[k, 0, 3:4].view(np.int32)[0]))
    assert all(x & SLAB for x in v), v
    three_walks(t, W, H, 2, 1)


def test_one_leaf_with_and_one_without_the_certificate():
    t = face_moved(copy_of(tables("cornell", W, H)))
    v, build = built(t)
    slab_list, slab_leaves = certificates(build)
    assert slab_list == 1 and slab_leaves in (1, 2), (slab_list, slab_leaves)
    assert all(x & PAIR and not x & SLAB for x in v), v
    three_walks(t, W, H, 2, 1, slab=False)
