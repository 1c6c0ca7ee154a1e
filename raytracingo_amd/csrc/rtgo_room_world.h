// rtgo_room_world.h -- the WORLD-axis form of a room's slab certificate (room_world, rtgo_device.h).  Plain C++, no HIP:
// the host derives it once per build from the six records of the up-front list's group (rtgo_analytic_host.h), a launch turns it into
// the words of PairWords (rtgo_capi.hip), and a stand-alone program can call both (tests/test_room_world_host.py).
//
// The slab certificate (rtgo_build.h, slab_certify) says: in the object frame of the group's first face -- rows R_0..R_2 of its
// record, q_a(x) = R_a.xyz . x + R_a.w -- the six faces are the planes q_a = lo_a, hi_a of one box.  The world form holds when each
// row is a world axis but for a residue: R_a.xyz = s_a e_j(a) + rho_a, the three j(a) distinct, rho_a without a j(a) component and
// |rho_a|_1 <= 2e-6 |s_a| (what slab_certify grants a face's normal).  Then
//     q_a(x) = s_a x_j + R_a.w + rho_a . x,
// so the plane q_a = b is the world plane x_j = (b - R_a.w) / s_a up to |rho_a . x| / |s_a| <= |rho_a|_1 |x|_inf / |s_a| -- a shift the
// margin can carry, because the steering only ever asks where a ray is at the parameter t* of a hit the reference accepts, and that
// point lies in the scene: |o + t* d|_inf <= |o|_inf + t* |d|_inf <= 3 reach (rtgo_capi.hip, cub_mu).  Crossings beyond the reach need
// no bound of their own: a candidate is dropped only when its own crossing lies past another axis' exit, and both sides of that compare
// are evaluated AT t*: "x(t*) within the widened frame slab of axis k" implies "x_k(t*) within the world slab widened by mu'", which in
// exact arithmetic is t* <= exit_k + mu' |1 / d_k|; likewise |t* - exit_a| <= mu' |1 / d_a| on the candidate's own axis.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

namespace rtgo {

struct RoomWorld {
    bool ok = false;
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};   // the room's planes per WORLD axis j
    int map = 0;                  // three bits per plane: the face's offset in the group; plane = 2 * world axis + (0: low, 1: high)
    float thr = 0.0f;             // |d_j| at or below this: the ray counts as parallel to the walls of world axis j (six single tests)
    float res[3] = {0, 0, 0};     // per world axis j = j(a): |rho_a|_1 / |s_a|
    float inv_s[3] = {0, 0, 0};   // ... and 1 / |s_a|: a frame unit of axis a in world units
    float rho = 1.0f;             // the slab certificate's rho: carries cub_mu into frame units
    float ext = 0.0f;             // the thinnest world slab
    float bmax = 0.0f;            // the largest |plane|
};

constexpr double kRoomWorldResidue = 2e-6;                       // |rho_a|_1 <= this * |s_a|
constexpr double kRoomWorldK = 64.0 * 5.9604644775390625e-8;     // the rounding allowance, as cub_mu's K: 64 * 2^-24

// rec: the six records of the group as the build wrote them (4 float4 = 16 floats each: rows 0..2 of M^-1, then (type, index, z, w) with
// the certificate's words in z, w: record a = 0..2 (lo_a, hi_a), record 3 (map, rho), record 4 (thr, 0)).  room / slab: the group holds
// the room and the slab certificate.
inline bool room_world_certify(const float (*rec)[16], bool room, bool slab, RoomWorld& out)
{
    out = RoomWorld();
    if (!room || !slab) return false;
    int map_f;
    std::memcpy(&map_f, &rec[3][14], sizeof map_f);
    const double rho = rec[3][15], thr_f = rec[4][14];
    if (!(rho >= 1.0 && rho < 1e6) || !(thr_f > 0.0 && thr_f < 1e30)) return false;
    int seen_axis = 0, seen_face = 0, map_w = 0;
    double thr_w = 0.0, ext = INFINITY, bmax = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double r[3] = {rec[0][4 * a + 0], rec[0][4 * a + 1], rec[0][4 * a + 2]}, w = rec[0][4 * a + 3];
        const double lo_f = rec[a][14], hi_f = rec[a][15];
        if (!(std::isfinite(r[0]) && std::isfinite(r[1]) && std::isfinite(r[2]) && std::isfinite(w) && std::isfinite(lo_f) && std::isfinite(hi_f))) return false;
        int j = 0;
        for (int k = 1; k < 3; ++k)
            if (std::fabs(r[k]) > std::fabs(r[j])) j = k;
        const double s = r[j], res1 = std::fabs(r[(j + 1) % 3]) + std::fabs(r[(j + 2) % 3]);
        if (!(std::fabs(s) > 0.0) || !(res1 <= kRoomWorldResidue * std::fabs(s)) || ((seen_axis >> j) & 1)) return false;
        seen_axis |= 1 << j;
        const bool neg = s < 0.0;
        const double p0 = (lo_f - w) / s, p1 = (hi_f - w) / s;
        out.lo[j] = (float)(neg ? p1 : p0);
        out.hi[j] = (float)(neg ? p0 : p1);
        out.res[j] = (float)(res1 / std::fabs(s));
        out.inv_s[j] = (float)(1.0 / std::fabs(s));
        if (!(out.lo[j] < out.hi[j]) || !std::isfinite(out.lo[j]) || !std::isfinite(out.hi[j])) return false;
        ext = std::fmin(ext, (double)out.hi[j] - (double)out.lo[j]);
        bmax = std::fmax(bmax, std::fmax(std::fabs((double)out.lo[j]), std::fabs((double)out.hi[j])));
        for (int side = 0; side < 2; ++side) {
            const int f = (map_f >> (3 * (2 * a + side))) & 7;
            if (f > 5 || ((seen_face >> f) & 1)) return false;
            seen_face |= 1 << f;
            map_w |= f << (3 * (2 * j + (side ^ (neg ? 1 : 0))));
        }
        // above the world threshold the frame component exceeds the frame threshold and has the world component's sign:
        // |R_a . d| >= |s_a| |d_j| - |rho_a|_1 |d|_inf, |d|_inf <= 1 but for the rounding of a normalisation
        thr_w = std::fmax(thr_w, (thr_f + 1.00001 * res1) / std::fabs(s));
    }
    if (seen_axis != 7 || seen_face != 63) return false;
    out.map = map_w;
    out.thr = std::nextafter((float)(thr_w * 1.000001), INFINITY);
    out.rho = (float)rho;
    out.ext = (float)ext;
    out.bmax = (float)bmax;
    // (a small room far from the origin: the rounding of the planes alone leaves no margin below 2 % of the thinnest slab at any reach)
    if (!std::isfinite(out.thr) || !(kRoomWorldK * 4.0 * bmax < 0.02 * ext)) return false;
    out.ok = true;
    return true;
}

// The margin of a launch in world units, or a negative number when the launch must not take the world form: cub_mu is the launch's
// cuboid margin (object-space y units of a face), reach its rays' reach.  Per world axis j = j(a): the frame margin cub_mu * rho and
// the residue's shift |rho_a|_1 * 3 reach, both over |s_a|; plus the rounding of the steering's own arithmetic -- the plane as a float
// (2^-24 |b|), the hardware reciprocal (1 ulp), noid and the fma (2^-24 each), the sums with w: under 2^-21 (|b| + |o|) as a position,
// K = 64 * 2^-24 on bmax + 3 reach leaves that eight times.  Refused unless below 2 % of the thinnest world slab.
inline float room_world_margin(const RoomWorld& w, float cub_mu, float reach)
{
    if (!w.ok || !(cub_mu > 0.0f) || !(reach >= 0.0f) || !std::isfinite(reach)) return -1.0f;
    double mu = 0.0;
    for (int j = 0; j < 3; ++j) mu = std::fmax(mu, (double)cub_mu * w.rho * w.inv_s[j] + (double)w.res[j] * 3.0 * reach);
    mu += kRoomWorldK * ((double)w.bmax + 3.0 * reach);
    const float m = std::nextafter((float)(mu * 1.000001), INFINITY);
    if (!(m > 0.0f) || !(m < 0.02f * w.ext)) return -1.0f;
    return m;
}

}  // namespace rtgo
