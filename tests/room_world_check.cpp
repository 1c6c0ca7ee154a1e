// The world-axis certificate of a room (csrc/rtgo_room_world.h) against a float64 evaluation in the FRAME form, on the CPU: a stand-alone
// program (tests/test_room_world_host.py builds it with -fsanitize=address,undefined -ffp-contract=off and runs it).
//
// For every accepted room it draws rays (origins within the reach, inside and outside the room; directions random, within 10x of the
// parallel threshold on an axis, and aimed at edges and corners), evaluates room_world's steering in float32 as the kernel does -- with
// each reciprocal as computed and one ulp to either side, v_rcp_f32 not being correctly rounded: 27 combinations -- and holds it to this:
// every face the ray leaves the room through whose float64 crossing point, in the frame of the room's first face, lies on the face
// widened by the frame margin is among the candidates, on the side the steering picks, or the lane is flat.  No exception is allowed.
// Prints, per room, the share of rays with more than one candidate; for cornell's room and random interior rays that share must stay
// below 5 %, in float32 and in a float64 evaluation of the same world form.
#include "rtgo_room_world.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using rtgo::RoomWorld;

namespace {

constexpr float kCuboidTolF = 1e-4f;              // rtgo_device.h, kCuboidTol
constexpr float kK = 64.0f * 5.9604645e-8f;       // the margins' rounding allowance
int g_fail = 0;
#define CHECK(c, ...)                            \
    do {                                         \
        if (!(c)) {                              \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);            \
            std::printf("\n");                   \
            ++g_fail;                            \
        }                                        \
    } while (0)

// ---- a room as the build describes it: the frame of its first face and the slab certificate's words
struct Frame {
    float R[3][4];        // rows 0..2 of the first face's inverse matrix
    float lo[3], hi[3];   // the box in the frame
    int map;              // plane 2a + side -> face offset
    float rho, thr;
    void records(float (*rec)[16]) const
    {
        std::memset(rec, 0, sizeof(float) * 6 * 16);
        for (int a = 0; a < 3; ++a)
            for (int k = 0; k < 4; ++k) rec[0][4 * a + k] = R[a][k];
        for (int a = 0; a < 3; ++a) {
            rec[a][14] = lo[a];
            rec[a][15] = hi[a];
        }
        std::memcpy(&rec[3][14], &map, sizeof map);
        rec[3][15] = rho;
        rec[4][14] = thr;
    }
    void finish()
    {
        float n1max = 0.0f;
        for (int a = 0; a < 3; ++a) n1max = std::fmax(n1max, std::fabs(R[a][0]) + std::fabs(R[a][1]) + std::fabs(R[a][2]));
        thr = 2e-5f * n1max;   // rtgo_build.h, slab_certify
    }
};

// ---- 3x4 float matrices, composed and inverted in float like the host's scene code
struct M34 {
    float m[3][4];
};
M34 mul(const M34& a, const M34& b)
{
    M34 r;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) {
            float s = j == 3 ? a.m[i][3] : 0.0f;
            for (int k = 0; k < 3; ++k) s += a.m[i][k] * b.m[k][j];
            r.m[i][j] = s;
        }
    return r;
}
M34 translate(float x, float y, float z) { return M34{{{1, 0, 0, x}, {0, 1, 0, y}, {0, 0, 1, z}}}; }
M34 scale(float x, float y, float z) { return M34{{{x, 0, 0, 0}, {0, y, 0, 0}, {0, 0, z, 0}}}; }
M34 rotate(float angle, int axis)   // about world axis 0 (x), 1 (y) or 2 (z)
{
    const float c = std::cos(angle), s = std::sin(angle);
    M34 r = scale(1, 1, 1);
    const int u = (axis + 1) % 3, v = (axis + 2) % 3;
    r.m[u][u] = c;
    r.m[u][v] = -s;
    r.m[v][u] = s;
    r.m[v][v] = c;
    return r;
}
M34 inverse(const M34& a)
{
    const float(*m)[4] = a.m;
    const float c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1], c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2], c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0];
    const float det = m[0][0] * c00 + m[0][1] * c01 + m[0][2] * c02, id = 1.0f / det;
    M34 r;
    r.m[0][0] = c00 * id;
    r.m[0][1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) * id;
    r.m[0][2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) * id;
    r.m[1][0] = c01 * id;
    r.m[1][1] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) * id;
    r.m[1][2] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) * id;
    r.m[2][0] = c02 * id;
    r.m[2][1] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) * id;
    r.m[2][2] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) * id;
    for (int i = 0; i < 3; ++i) r.m[i][3] = -(r.m[i][0] * m[0][3] + r.m[i][1] * m[1][3] + r.m[i][2] * m[2][3]);
    return r;
}

// the six walls of a room as the scene code's make_room composes them (one-sided unit rectangles, normal +y in object space, facing
// inwards), optionally turned as a whole about the world y axis; `first`: the wall that comes first in the group
bool room_frame(float hx, float hy, float hz, float turn, int first, Frame& f)
{
    const float pi = 3.14159265358979323846f, sx = 2 * hx, sy = 2 * hy, sz = 2 * hz;
    M34 w[6] = {mul(mul(translate(0, 0, -hz), rotate(pi / 2, 0)), scale(sx, 1, sy)), mul(mul(translate(0, 0, hz), rotate(-pi / 2, 0)), scale(sx, 1, sy)),
                mul(mul(translate(-hx, 0, 0), rotate(-pi / 2, 2)), scale(sy, 1, sz)), mul(mul(translate(hx, 0, 0), rotate(pi / 2, 2)), scale(sy, 1, sz)),
                mul(mul(translate(0, hy, 0), rotate(pi, 2)), scale(sx, 1, sz)),       mul(translate(0, -hy, 0), scale(sx, 1, sz))};
    if (turn != 0.0f)
        for (M34& m : w) m = mul(rotate(turn, 1), m);
    std::swap(w[0], w[first]);
    const M34 inv = inverse(w[0]);
    std::memcpy(f.R, inv.m, sizeof f.R);
    for (int a = 0; a < 3; ++a) {
        f.lo[a] = INFINITY;
        f.hi[a] = -INFINITY;
    }
    auto to_frame = [&](float x, float y, float z, float* q) {
        for (int a = 0; a < 3; ++a) q[a] = f.R[a][0] * x + f.R[a][1] * y + f.R[a][2] * z + f.R[a][3];
    };
    for (const M34& m : w)
        for (int c = 0; c < 4; ++c) {
            const float u = (c & 1) ? 0.5f : -0.5f, v = (c & 2) ? 0.5f : -0.5f;
            float q[3];
            to_frame(m.m[0][0] * u + m.m[0][2] * v + m.m[0][3], m.m[1][0] * u + m.m[1][2] * v + m.m[1][3], m.m[2][0] * u + m.m[2][2] * v + m.m[2][3], q);
            for (int a = 0; a < 3; ++a) {
                f.lo[a] = std::fmin(f.lo[a], q[a]);
                f.hi[a] = std::fmax(f.hi[a], q[a]);
            }
        }
    f.map = 0;
    f.rho = 1.0f;
    int filled = 0;
    for (int k = 0; k < 6; ++k) {
        float q[3];
        to_frame(w[k].m[0][3], w[k].m[1][3], w[k].m[2][3], q);
        int axis = -1, side = 0;
        for (int a = 0; a < 3; ++a) {
            const float e = f.hi[a] - f.lo[a], dl = std::fabs(q[a] - f.lo[a]), dh = std::fabs(f.hi[a] - q[a]);
            if (std::fmin(dl, dh) <= 1e-3f * e) {
                axis = a;
                side = dl <= dh ? 0 : 1;
            }
        }
        if (axis < 0) return false;
        filled |= 1 << (2 * axis + side);
        f.map |= k << (3 * (2 * axis + side));
        f.rho = std::fmax(f.rho, std::fabs(f.R[axis][0] * w[k].m[0][1] + f.R[axis][1] * w[k].m[1][1] + f.R[axis][2] * w[k].m[2][1]));
    }
    f.finish();
    return filled == 63;
}

// a synthesized frame: row a = s[a] e_perm[a] + a residue of L1 norm resid * |s[a]| on the other two components, over the world box
// [wlo, whi]; shear: added to row 0's second component as it is
Frame synth_frame(const int* perm, const float* s, float resid, float shear, const float* wlo, const float* whi, std::mt19937& rng)
{
    Frame f;
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    for (int a = 0; a < 3; ++a) {
        const int j = perm[a];
        const float split = U(rng), r1 = resid * std::fabs(s[a]) * split, r2 = resid * std::fabs(s[a]) * (1.0f - split) * 0.999f;
        f.R[a][j] = s[a];
        f.R[a][(j + 1) % 3] = (U(rng) < 0.5f ? -r1 : r1) * 0.999f;
        f.R[a][(j + 2) % 3] = U(rng) < 0.5f ? -r2 : r2;
        f.R[a][3] = 0.25f * (float)(a - 1);
        const float p0 = s[a] * wlo[j] + f.R[a][3], p1 = s[a] * whi[j] + f.R[a][3];
        f.lo[a] = std::fmin(p0, p1);
        f.hi[a] = std::fmax(p0, p1);
    }
    f.R[0][(perm[0] + 1) % 3] += shear;
    const int faces[6] = {3, 0, 5, 1, 4, 2};
    f.map = 0;
    for (int k = 0; k < 6; ++k) f.map |= faces[k] << (3 * k);
    f.rho = 1.0f;
    f.finish();
    return f;
}

float ulp_step(float x, int k) { return k == 0 ? x : std::nextafter(x, k > 0 ? INFINITY : -INFINITY); }

struct Tally {
    long rays = 0, flat = 0, multi = 0, multi64 = 0, exceptions = 0, faces = 0;
};

// one ray: room_world's steering in float32 (rtgo_device.h) under the 27 nudges of the reciprocal, held to the float64 frame form
void one_ray(const Frame& f, const RoomWorld& w, float mu_w, float mu_frame, const float* o, const float* d, Tally& t)
{
    // the faces the float64 frame form says the ray may hit: plane (a, side), left through it, crossing point on the widened face
    int want_axis[6], want_side[6], n_want = 0;
    double da[3], oa[3];
    for (int a = 0; a < 3; ++a) {
        da[a] = (double)f.R[a][0] * d[0] + (double)f.R[a][1] * d[1] + (double)f.R[a][2] * d[2];
        oa[a] = (double)f.R[a][0] * o[0] + (double)f.R[a][1] * o[1] + (double)f.R[a][2] * o[2] + (double)f.R[a][3];
    }
    int j_of[3], neg[3];
    for (int a = 0; a < 3; ++a) {
        int j = 0;
        for (int k = 1; k < 3; ++k)
            if (std::fabs(f.R[a][k]) > std::fabs(f.R[a][j])) j = k;
        j_of[a] = j;
        neg[a] = f.R[a][j] < 0.0f;
    }
    for (int a = 0; a < 3; ++a)
        for (int side = 0; side < 2; ++side) {
            if (!(side ? da[a] > 0.0 : da[a] < 0.0)) continue;
            const double ts = ((side ? (double)f.hi[a] : (double)f.lo[a]) - oa[a]) / da[a];
            if (!std::isfinite(ts)) continue;
            bool on = true;
            for (int k = 0; k < 3; ++k)
                if (k != a) {
                    const double q = oa[k] + ts * da[k];
                    on = on && q >= (double)f.lo[k] - mu_frame && q <= (double)f.hi[k] + mu_frame;
                }
            if (on) {
                want_axis[n_want] = j_of[a];
                want_side[n_want] = side ^ neg[a];
                ++n_want;
            }
        }
    t.faces += n_want;
    bool flat = false;
    for (int j = 0; j < 3; ++j) flat = flat || std::fabs(d[j]) <= w.thr;
    float id0[3];
    for (int j = 0; j < 3; ++j) id0[j] = 1.0f / d[j];   // (correctly rounded: the hardware's is within an ulp of it)
    bool multi = false;
    if (!flat) {
        for (int n = 0; n < 27; ++n) {
            const int nud[3] = {n % 3 - 1, (n / 3) % 3 - 1, n / 9 - 1};
            float tp[3], ws[3], X = INFINITY;
            for (int j = 0; j < 3; ++j) {
                const float id = std::fmin(std::fmax(ulp_step(id0[j], nud[j]), -1e30f), 1e30f);
                const float noid = -(o[j] * id);
                tp[j] = std::fmax(std::fmaf(w.lo[j], id, noid), std::fmaf(w.hi[j], id, noid));
                ws[j] = mu_w * id;
                X = std::fmin(X, tp[j] + std::fabs(ws[j]));
            }
            bool cand[3];
            int side[3], nc = 0;
            for (int j = 0; j < 3; ++j) {
                cand[j] = !(X < tp[j] - std::fabs(ws[j]));
                side[j] = std::signbit(ws[j]) ? 0 : 1;
                nc += cand[j] ? 1 : 0;
            }
            if (n == 13 && nc > 1) multi = true;
            for (int k = 0; k < n_want; ++k)
                if (!(cand[want_axis[k]] && side[want_axis[k]] == want_side[k])) {
                    if (t.exceptions < 5)
                        std::printf("  exception: o %.9g %.9g %.9g d %.9g %.9g %.9g wants axis %d side %d, nudge %d: cand %d %d %d\n", o[0], o[1], o[2], d[0], d[1], d[2],
                                    want_axis[k], want_side[k], n, cand[0], cand[1], cand[2]);
                    ++t.exceptions;
                }
        }
        // the same world form in float64: what the construction (margins, no entry side) lets through, rounding apart
        double X = INFINITY, tp[3], wd[3];
        for (int j = 0; j < 3; ++j) {
            const double id = 1.0 / (double)d[j];
            tp[j] = std::fmax(((double)w.lo[j] - o[j]) * id, ((double)w.hi[j] - o[j]) * id);
            wd[j] = std::fabs(mu_w * id);
            X = std::fmin(X, tp[j] + wd[j]);
        }
        int nc = 0;
        for (int j = 0; j < 3; ++j) nc += !(X < tp[j] - wd[j]) ? 1 : 0;
        t.multi64 += nc > 1 ? 1 : 0;
    }
    t.rays += 1;
    t.flat += flat ? 1 : 0;
    t.multi += multi ? 1 : 0;
}

void normalise(float* d)
{
    const float l = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (l > 0.0f)
        for (int k = 0; k < 3; ++k) d[k] /= l;
}

// accepted room: the certificate, its outputs against the frame, and the rays
void accepted(const std::string& name, const Frame& f, bool cornell, std::mt19937& rng)
{
    float rec[6][16];
    f.records(rec);
    RoomWorld w;
    const bool ok = rtgo::room_world_certify(rec, true, true, w);
    CHECK(ok, "%s: the certificate was refused", name.c_str());
    if (!ok) return;
    RoomWorld none;
    CHECK(!rtgo::room_world_certify(rec, false, true, none) && !rtgo::room_world_certify(rec, true, false, none), "%s: accepted without the room or slab certificate", name.c_str());
    // the map, re-indexed: the same face for the same plane
    for (int a = 0; a < 3; ++a) {
        int j = 0;
        for (int k = 1; k < 3; ++k)
            if (std::fabs(f.R[a][k]) > std::fabs(f.R[a][j])) j = k;
        for (int side = 0; side < 2; ++side) {
            const int ws = side ^ (f.R[a][j] < 0.0f ? 1 : 0);
            CHECK(((w.map >> (3 * (2 * j + ws))) & 7) == ((f.map >> (3 * (2 * a + side))) & 7), "%s: map of frame plane %d side %d", name.c_str(), a, side);
        }
        CHECK(w.thr * std::fabs(f.R[a][j]) >= f.thr, "%s: the world threshold is laxer than the frame's on axis %d", name.c_str(), a);
    }
    const float reach = 2.0f * w.bmax;
    float n1max = 0.0f, wmax = 0.0f;
    for (int a = 0; a < 3; ++a) {
        n1max = std::fmax(n1max, std::fabs(f.R[a][0]) + std::fabs(f.R[a][1]) + std::fabs(f.R[a][2]));
        wmax = std::fmax(wmax, std::fabs(f.R[a][3]));
    }
    const float cub_mu = kCuboidTolF + kK * (2.0f * n1max * 3.0f * reach + 2.0f * wmax + 2.0f);   // (rtgo_capi.hip, walk_params: its shape, generous coefficients)
    const float mu_w = rtgo::room_world_margin(w, cub_mu, reach);
    CHECK(mu_w > 0.0f && mu_w < 0.02f * w.ext, "%s: no margin at reach %g (%g)", name.c_str(), reach, mu_w);
    if (!(mu_w > 0.0f)) return;
    const float mu_frame = cub_mu * f.rho;   // (cuboid_slab: mu = mu_launch * rho)
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    auto gauss_dir = [&](float* d) {
        std::normal_distribution<float> N(0.0f, 1.0f);
        do {
            for (int k = 0; k < 3; ++k) d[k] = N(rng);
        } while (d[0] * d[0] + d[1] * d[1] + d[2] * d[2] < 1e-6f);
        normalise(d);
    };
    Tally all, interior;
    const long n_rays = 120000;
    for (long i = 0; i < n_rays; ++i) {
        float o[3], d[3];
        const bool inside = (i & 1) == 0;
        for (int j = 0; j < 3; ++j) o[j] = inside ? w.lo[j] + (w.hi[j] - w.lo[j]) * U(rng) : reach * (2.0f * U(rng) - 1.0f);
        const int kind = (int)(i % 6);
        gauss_dir(d);
        if (kind == 2 || kind == 3) {   // within 10x of the parallel threshold on one axis (kind 2) or two (kind 3)
            const int j0 = (int)(U(rng) * 3.0f) % 3;
            for (int q = 0; q < (kind == 2 ? 1 : 2); ++q) {
                const float v = w.thr * std::pow(10.0f, 2.0f * U(rng) - 1.0f);
                d[(j0 + q) % 3] = U(rng) < 0.5f ? -v : v;
            }
            if (U(rng) < 0.7f) normalise(d);
        } else if (kind >= 4) {   // aimed at an edge (kind 4) or a corner (kind 5), within a few margins of it
            float target[3];
            const int free_axis = kind == 4 ? (int)(U(rng) * 3.0f) % 3 : -1;
            for (int j = 0; j < 3; ++j) {
                target[j] = j == free_axis ? w.lo[j] + (w.hi[j] - w.lo[j]) * U(rng) : (U(rng) < 0.5f ? w.lo[j] : w.hi[j]);
                if (j != free_axis) target[j] += mu_w * 4.0f * (2.0f * U(rng) - 1.0f);
                d[j] = target[j] - o[j];
            }
            normalise(d);
            if (!(std::fabs(d[0]) + std::fabs(d[1]) + std::fabs(d[2]) > 0.5f)) gauss_dir(d);
        }
        one_ray(f, w, mu_w, mu_frame, o, d, all);
        if (inside && kind < 2) one_ray(f, w, mu_w, mu_frame, o, d, interior);
    }
    std::printf("%-34s rays %ld, faces wanted %ld, flat %.3f %%, more than one candidate %.3f %% (float64 %.3f %%); random interior rays %ld: %.3f %% (float64 %.3f %%); margin %g of a thinnest slab %g, threshold %g; exceptions %ld\n",
                name.c_str(), all.rays, all.faces, 100.0 * all.flat / all.rays, 100.0 * all.multi / all.rays, 100.0 * all.multi64 / all.rays, interior.rays,
                100.0 * interior.multi / interior.rays, 100.0 * interior.multi64 / interior.rays, mu_w, w.ext, w.thr, all.exceptions);
    CHECK(all.rays >= 100000, "%s: too few rays", name.c_str());
    CHECK(all.faces > all.rays / 4, "%s: the float64 form wanted hardly any face (%ld)", name.c_str(), all.faces);
    CHECK(all.exceptions == 0, "%s: %ld exceptions", name.c_str(), all.exceptions);
    if (cornell) {
        CHECK(interior.multi * 20 < interior.rays, "%s: more than one candidate on %.2f %% of the random interior rays", name.c_str(), 100.0 * interior.multi / interior.rays);
        CHECK(interior.multi64 * 20 < interior.rays, "%s: float64: more than one candidate on %.2f %% of the random interior rays", name.c_str(), 100.0 * interior.multi64 / interior.rays);
    }
}

void refused(const std::string& name, const Frame& f, float reach)
{
    float rec[6][16];
    f.records(rec);
    RoomWorld w;
    const bool ok = rtgo::room_world_certify(rec, true, true, w);
    const float mu = ok ? rtgo::room_world_margin(w, kCuboidTolF, reach) : -1.0f;
    std::printf("%-34s certificate %d, margin %g\n", name.c_str(), ok ? 1 : 0, mu);
    CHECK(!(mu > 0.0f), "%s: accepted", name.c_str());
}

}  // namespace

int main()
{
    std::mt19937 rng(20250117u);
    const char* wall[6] = {"back", "front", "left", "right", "top", "bottom"};
    Frame f;
    // cornell's room as the scene code gives it (its walls in insertion order: the back wall first), and with each wall first
    for (int first = 0; first < 6; ++first) {
        CHECK(room_frame(4.0f, 4.0f, 4.0f, 0.0f, first, f), "cornell's room, %s wall first: no frame", wall[first]);
        accepted(std::string("cornell's room, first wall ") + wall[first], f, true, rng);
    }
    CHECK(room_frame(8.0f, 4.0f, 8.0f, 0.0f, 0, f), "the wide room: no frame");
    accepted("the 16 x 8 x 16 room", f, false, rng);
    CHECK(room_frame(4.0f, 4.0f, 4.0f, 1e-6f, 0, f), "the room turned by 1e-6: no frame");
    accepted("cornell's room turned by 1e-6 rad", f, true, rng);
    const float wlo[3] = {-4.0f, -3.0f, -5.0f}, whi[3] = {4.0f, 6.0f, 2.0f};
    const int ident[3] = {0, 1, 2}, cyc[3] = {2, 0, 1}, swp[3] = {1, 0, 2};
    const float pos[3] = {0.125f, 1.0f, 0.25f}, negs[3] = {-0.125f, 1.0f, -0.25f}, neg1[3] = {0.125f, -1.0f, 0.125f};
    accepted("synthesized, no residue", synth_frame(ident, pos, 0.0f, 0.0f, wlo, whi, rng), false, rng);
    accepted("synthesized, negative s (0 and 2)", synth_frame(ident, negs, 1e-7f, 0.0f, wlo, whi, rng), false, rng);
    accepted("synthesized, negative s (1)", synth_frame(ident, neg1, 1e-7f, 0.0f, wlo, whi, rng), false, rng);
    accepted("synthesized, axes 2 0 1", synth_frame(cyc, pos, 1e-7f, 0.0f, wlo, whi, rng), false, rng);
    accepted("synthesized, axes 1 0 2, negative", synth_frame(swp, negs, 1e-7f, 0.0f, wlo, whi, rng), false, rng);
    accepted("synthesized, residue 1e-7", synth_frame(ident, pos, 1e-7f, 0.0f, wlo, whi, rng), false, rng);
    accepted("synthesized, residue 1e-6", synth_frame(cyc, negs, 1e-6f, 0.0f, wlo, whi, rng), false, rng);
    // refused
    refused("residue 1e-3", synth_frame(ident, pos, 1e-3f, 0.0f, wlo, whi, rng), 12.0f);
    refused("a sheared frame", synth_frame(ident, pos, 0.0f, 0.02f, wlo, whi, rng), 12.0f);
    CHECK(room_frame(4.0f, 4.0f, 4.0f, 1e-3f, 0, f), "the room turned by 1e-3: no frame");
    refused("cornell's room turned by 1e-3 rad", f, 12.0f);
    const float tlo[3] = {100.0f, 100.0f, 100.0f}, thi[3] = {100.001f, 100.001f, 100.001f}, big[3] = {1000.0f, 1000.0f, 1000.0f};
    refused("a 1e-3 room 100 units out", synth_frame(ident, big, 0.0f, 0.0f, tlo, thi, rng), 101.0f);
    {   // non-finite words
        Frame g = synth_frame(ident, pos, 0.0f, 0.0f, wlo, whi, rng);
        g.hi[1] = INFINITY;
        refused("an infinite bound", g, 12.0f);
        g = synth_frame(ident, pos, 0.0f, 0.0f, wlo, whi, rng);
        g.R[2][3] = NAN;
        refused("a NaN in a row", g, 12.0f);
        g = synth_frame(ident, pos, 0.0f, 0.0f, wlo, whi, rng);
        g.map = 0;
        refused("a map that names one face six times", g, 12.0f);
    }
    if (g_fail) {
        std::printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
