"""oracle_intersect held to tests/analytic_ref64.py, a float64 reference written from the geometry, one primitive at a time: random
families per type, plain and sheared, and hand-placed rays whose answers are known.  Every other check of the sphere, cylinder, disk and
rectangle intersectors compares float32 code with float32 code restated from the same lines; this is their anchor outside those lines, and
tests/test_trace_rays_float64.py holds the device to the same reference and the same constants."""
import ctypes as C

import numpy as np
import pytest

import analytic_ref64 as A

NAMES = {A.CYLINDER: "cylinder", A.DISK: "disk", A.RECTANGLE: "rectangle", A.SPHERE: "sphere"}
# The oracle's largest deviations from the float64 reference over the clear rays of the eight families below, measured on the CPU
# (DESIGN.md 4); plain and sheared together.  Hit point: |t32 - t64| |d| in units of 2^-23 reach, reach = |o - centre| + ||M3x3||_2.
# Normal: the sine of the angle between the two.  The bounds are 4 x these, and the device is held to the same constants.
MEASURED_T_UNITS = {A.CYLINDER: 112.0, A.DISK: 72.0, A.RECTANGLE: 33.0, A.SPHERE: 89.0}
MEASURED_N_SINE = {A.CYLINDER: 6.0e-4, A.DISK: 7.5e-8, A.RECTANGLE: 6.7e-8, A.SPHERE: 5.4e-4}
T_BOUND_UNITS = {k: 4 * v for k, v in MEASURED_T_UNITS.items()}
N_BOUND_SINE = {k: 4 * v for k, v in MEASURED_N_SINE.items()}
UNCLEAR_CAP = 0.20
MATRICES, RAYS_PER_MATRIX = 40, 100     # 4000 rays a family
UNIT = 2.0 ** -23
# ||M inv32(M) - I||_inf <= 64 x 2^-23 x cond_inf(M): the cofactor inverse sums three products of three factors per entry and scales by a
# reciprocal, a few roundings each, and the residual's row sums add four such entries against M's row
INVERSE_BOUND = 64 * UNIT


def oracle_hits(oracle, ty, M, o, d):
    """oracle_intersect of one primitive for every ray: hit [n] bool, t [n] float32, n [n, 3] float32; no window (the intersector's own
    thresholds only)"""
    L = oracle.lib()
    p = oracle.Prim()
    p.type = int(ty)
    p.M[:] = np.asarray(M, np.float32).reshape(16).tolist()
    o, d = oracle.f32(o), oracle.f32(d)
    hit, t, n = np.zeros(len(o), bool), np.zeros(len(o), np.float32), np.zeros((len(o), 3), np.float32)
    tv, nv = C.c_float(0), (C.c_float * 3)()
    for k in range(len(o)):
        if L.oracle_intersect(C.byref(p), oracle.fptr(o[k]), oracle.fptr(d[k]), C.byref(tv), nv):
            hit[k], t[k], n[k] = True, tv.value, (nv[0], nv[1], nv[2])
    return hit, t, n


def deviations(ty, M, o, d, ref_t, ref_n, t, n):
    """hit-point deviation in units of 2^-23 reach and the normals' sine, per ray (rays both sides hit)"""
    dl = np.linalg.norm(np.asarray(d, np.float64), axis=-1)
    return np.abs(np.asarray(t, np.float64) - ref_t) * dl / (UNIT * A.reach(M, o)), A.normal_sine(n, ref_n)


def one_primitive(ty, M, o, d):
    """the reference for a single primitive without a window: hit, t, n, clear"""
    r = A.closest([ty], np.asarray(M)[None], o, d, 0.0, np.inf)
    return r["prim"] == 0, r["t"], r["n"], r["clear"]


def inverse_residual(M, inv):
    """||M inv - I||_inf and cond_inf(M) for 4 x 4 float64 matrices (inv: the float32 inverse under test, widened)"""
    norm = lambda a: np.abs(a).sum(1).max()
    return norm(M @ inv - np.eye(4)), norm(M) * norm(np.linalg.inv(M))


_family = {}


def family(oracle, ty, sheared):
    """the family's rays, the oracle's answers and the reference's, computed once"""
    key = (ty, sheared)
    if key not in _family:
        rng = np.random.RandomState(1000 + 10 * ty + int(sheared))
        rows = []
        for _ in range(MATRICES):
            M = A.random_matrix(rng, sheared)
            o, d = A.aimed_rays(rng, ty, M, RAYS_PER_MATRIX)
            hit, t, n = oracle_hits(oracle, ty, M, o, d)
            rhit, rt, rn, clear = one_primitive(ty, M, o, d)
            both = hit & rhit
            dt, dn = np.zeros(len(o)), np.zeros(len(o))
            dt[both], dn[both] = deviations(ty, M, o[both], d[both], rt[both], rn[both], t[both], n[both])
            rows.append((hit, rhit, clear, dt, dn, (n * rn).sum(-1)))
        _family[key] = [np.concatenate(c) for c in zip(*rows)]
    return _family[key]


@pytest.mark.parametrize("sheared", [False, True], ids=["plain", "sheared"])
@pytest.mark.parametrize("ty", [A.SPHERE, A.CYLINDER, A.DISK, A.RECTANGLE], ids=lambda ty: NAMES[ty])
def test_random_family(oracle, ty, sheared):
    hit, rhit, clear, dt, dn, cos = family(oracle, ty, sheared)
    both = clear & hit & rhit
    wrong = np.nonzero(clear & (hit != rhit))[0]
    print("%s %s: %d rays, %d hit, unclear %.4f, wrong decisions on clear rays %d, hit point %.1f units, normal sine %.3g"
          % (NAMES[ty], "sheared" if sheared else "plain", len(hit), rhit.sum(), 1 - clear.mean(), len(wrong), dt[both].max(initial=0), dn[both].max(initial=0)))
    assert 1 - clear.mean() <= UNCLEAR_CAP
    assert rhit[clear].sum() >= 200 and (~rhit[clear]).sum() >= 200     # the family exercises both answers
    assert len(wrong) == 0, wrong[:10]
    assert dt[both].max() <= T_BOUND_UNITS[ty], dt[both].max()
    assert dn[both].max() <= N_BOUND_SINE[ty] and (cos[both] > 0).all(), dn[both].max()


def check_known(name, ty, M, o, d, answer, hit, t, n):
    """one hand-placed ray: the float64 reference gives the hand-computed answer, and (hit, t, n) -- the code under test -- agrees with the
    reference within the bounds"""
    rhit, rt, rn, _ = one_primitive(ty, M, o[None], d[None])
    assert np.isfinite(n).all() and np.isfinite(t), name
    if answer is None:
        assert not rhit[0], name
        assert not hit, name
        return
    t_hand, n_obj = answer
    n_hand = np.linalg.inv(np.asarray(M, np.float64).reshape(4, 4))[:3, :3].T @ np.asarray(n_obj, np.float64)
    # (the world ray is rounded to float32 after it was placed: 1e-3 covers that, and no rule's other branch lands that close)
    assert rhit[0] and abs(rt[0] - t_hand) <= 1e-3 * t_hand and A.normal_sine(n_hand, rn[0]) <= 1e-3 and n_hand @ rn[0] > 0, (name, rt[0])
    assert hit, name
    dt, dn = deviations(ty, M, o[None], d[None], rt, rn, np.array([t]), np.asarray(n)[None])
    assert dt[0] <= T_BOUND_UNITS[ty] and dn[0] <= N_BOUND_SINE[ty] and np.dot(n, rn[0]) > 0, (name, dt[0], dn[0])


@pytest.mark.parametrize("which", ["identity", "sheared"])
def test_known_answers(oracle, which):
    M = A.IDENTITY if which == "identity" else A.SHEARED
    for name, ty, o_obj, d_obj, answer in A.KNOWN:
        o, d = A.to_world(M, o_obj, d_obj)
        hit, t, n = oracle_hits(oracle, ty, M, o[None], d[None])
        check_known(name, ty, M, o, d, answer, hit[0], t[0], n[0])


def check_units(ty, M, o, d, scale, hit, t, t_unscaled):
    """(o, s d): t / s within the bound, or a miss that the float64 reference shares.  Returns whether it hit."""
    rhit, rt, rn, _ = one_primitive(ty, M, o[None], d[None])
    assert bool(hit) == bool(rhit[0]), (NAMES[ty], scale)
    if hit:
        dt, _ = deviations(ty, M, o[None], d[None], rt, rn, np.array([t]), rn)
        assert dt[0] <= T_BOUND_UNITS[ty], (NAMES[ty], scale, dt[0])
        assert abs(rt[0] * scale - t_unscaled) <= 1e-3 * t_unscaled, (NAMES[ty], scale, rt[0])
    return bool(hit)


@pytest.mark.parametrize("which", ["identity", "sheared"])
def test_t_is_in_units_of_dir(oracle, which):
    M = A.IDENTITY if which == "identity" else A.SHEARED
    outcomes = set()
    for ty, o_obj, d_obj in A.UNITS:
        t1 = one_primitive(ty, M, *[v[None] for v in A.to_world(M, o_obj, d_obj)])[1][0]
        assert np.isfinite(t1), NAMES[ty]
        for s in A.SCALES:
            o, d = A.to_world(M, o_obj, np.asarray(d_obj, np.float64) * s)
            hit, t, n = oracle_hits(oracle, ty, M, o[None], d[None])
            outcomes.add(check_units(ty, M, o, d, s, hit[0], t[0], t1))
    assert outcomes == {True, False}


@pytest.mark.parametrize("sheared", [False, True], ids=["plain", "sheared"])
def test_inverse_residual(oracle, sheared):
    """oracle_mat_inverse on the families' matrices (the device's inverses are held to the same bound in test_trace_rays_float64.py)"""
    rng = np.random.RandomState(77 + int(sheared))
    worst = 0.0
    for _ in range(2000):
        M = A.random_matrix(rng, sheared)
        inv = np.zeros(16, np.float32)
        oracle.lib().oracle_mat_inverse(oracle.fptr(M), oracle.fptr(inv))
        res, cond = inverse_residual(M.astype(np.float64).reshape(4, 4), inv.astype(np.float64).reshape(4, 4))
        worst = max(worst, res / cond)
        assert res <= INVERSE_BOUND * cond, (M, res, cond)
    print("%s: largest ||M inv - I|| / cond = %.3g = %.2f x 2^-23 (bound 64)" % ("sheared" if sheared else "plain", worst, worst / UNIT))
