/*
 * rtgo_oracle_whitted.c -- CPU ORACLE of the "whitted" triangle path.  TEST INFRASTRUCTURE ONLY (see rtgo_oracle.h).
 *
 * Plain-C restatement of the reference's cuda/whitted.cu -- __raygen__pinhole (:183-240), __miss__constant_radiance
 * (:243-246), __closesthit__occlusion (:249-252), __closesthit__radiance (:255-337), the GGX helpers (:49-89), make_color
 * (:164-173) -- of getLocalGeometry for triangle meshes (cuda/LocalGeometry.h:55-141), and of tex2D<float4> on the texture objects
 * sutil::Scene::addSampler makes (sutil/Scene.cpp:505-538; the filtering arithmetic is the CUDA programming guide's, "Texture Fetching").
 *
 * PINNING STATUS: tea<4> / rnd are held to the reference's own cuda/random.h through oracle/_ref (tests/golden/ref_blocks.json).
 * Everything else here is PARITY UNPINNED: whitted.cu includes <optix.h> (absent from this image), no program of the reference
 * ever launches it (engine/ never instantiates sutil::Scene), and the reference holds no fixture for it.  Triangle
 * intersection itself is OptiX's built-in (closed): the Moeller-Trumbore statement below is this project's definition, shared
 * operation for operation with the device code (raytracingo_amd/csrc/rtgo_whitted.h).  Traversal is brute force in triangle
 * order: the closest hit is the smallest t, the lowest triangle index on ties.  What this file computes after the hit is held to a float64
 * statement written from whitted.cu and the definitions, not from this text (tests/whitted_ref64.py, tests/test_oracle_whitted_float64.py).
 */
#include "rtgo_oracle.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

typedef struct { float x, y, z; } w3;
static inline w3 W3(float x, float y, float z) { w3 r = { x, y, z }; return r; }
static inline w3 wadd(w3 a, w3 b) { return W3(a.x + b.x, a.y + b.y, a.z + b.z); }
static inline w3 wsub(w3 a, w3 b) { return W3(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline w3 wmul(w3 a, w3 b) { return W3(a.x * b.x, a.y * b.y, a.z * b.z); }
static inline w3 wscale(w3 a, float s) { return W3(a.x * s, a.y * s, a.z * s); }
static inline w3 wneg(w3 a) { return W3(-a.x, -a.y, -a.z); }
static inline float wdot(w3 a, w3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }                 /* vec_math.h:523-526 */
static inline w3 wcross(w3 a, w3 b) { return W3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); } /* :529-532 */
static inline float wlength(w3 v) { return sqrtf(wdot(v, v)); }                                    /* :535-538 */
static inline w3 wnormalize(w3 v) { float inv = 1.0f / sqrtf(wdot(v, v)); return wscale(v, inv); } /* :541-545 */
static inline float wclamp(float f, float a, float b) { return fmaxf(a, fminf(f, b)); }            /* :115-118 */
static inline w3 wld(const float* p, uint32_t i) { return W3(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }

/* tea<4>, cuda/random.h:30-45 */
uint32_t oracle_tea4(uint32_t v0, uint32_t v1)
{
    uint32_t s0 = 0;
    for (int n = 0; n < 4; ++n) {
        s0 += 0x9e3779b9u;
        v0 += ((v1 << 4) + 0xa341316cu) ^ (v1 + s0) ^ ((v1 >> 5) + 0xc8013ea4u);
        v1 += ((v0 << 4) + 0xad90777du) ^ (v0 + s0) ^ ((v0 >> 5) + 0x7e95761eu);
    }
    return v0;
}

/* Moeller-Trumbore, two-sided; hit iff tmin < t < tmax.  p0..p2, o, d: 3 floats each. */
int oracle_tri_intersect(const float* p0, const float* p1, const float* p2, const float* o, const float* d, float tmin, float tmax,
                         float* t_out, float* u_out, float* v_out)
{
    const w3 P0 = wld(p0, 0), P1 = wld(p1, 0), P2 = wld(p2, 0), O = wld(o, 0), D = wld(d, 0);
    const w3 e1 = wsub(P1, P0), e2 = wsub(P2, P0);
    const w3 pv = wcross(D, e2);
    const float det = wdot(e1, pv);
    if (det == 0.0f) return 0;
    const float inv = 1.0f / det;
    const w3 tv = wsub(O, P0);
    const float u = wdot(tv, pv) * inv;
    if (u < 0.0f || u > 1.0f) return 0;
    const w3 qv = wcross(tv, e1);
    const float v = wdot(D, qv) * inv;
    if (v < 0.0f || u + v > 1.0f) return 0;
    const float t = wdot(e2, qv) * inv;
    if (!(t > tmin && t < tmax)) return 0;
    *t_out = t;
    *u_out = u;
    *v_out = v;
    return 1;
}

/* tex2D<float4>( tex, u, v ): cudaReadModeNormalizedFloat, normalizedCoords, and -- addSampler compares its CUDA enum arguments with GL
   constants (Scene.cpp:517-524), so always -- cudaAddressModeWrap and cudaFilterModeLinear.  CUDA programming guide, linear filtering:
   xB = u N - 0.5, i = floor(xB), alpha = frac(xB) in 1.8 fixed point (rounded to nearest here: the hardware's rounding is not published,
   PARITY UNPINNED), tex = (1-a)(1-b) T[i,j] + a(1-b) T[i+1,j] + (1-a) b T[i,j+1] + a b T[i+1,j+1], indices wrapped.  Operation order
   shared with the device code (rtgo_whitted.h, tex2d). */
void oracle_tex2d(const oracle_tex* t, float u, float v, float* rgba)
{
    const float xb = u * (float)t->w - 0.5f, yb = v * (float)t->h - 0.5f;
    const float fx = floorf(xb), fy = floorf(yb);
    const float a = floorf((xb - fx) * 256.0f + 0.5f) * (1.0f / 256.0f), b = floorf((yb - fy) * 256.0f + 0.5f) * (1.0f / 256.0f);
    const int w = (int)t->w, h = (int)t->h;
    int i0 = (int)fx % w, j0 = (int)fy % h;
    i0 += i0 < 0 ? w : 0;
    j0 += j0 < 0 ? h : 0;
    const int i1 = i0 + 1 == w ? 0 : i0 + 1, j1 = j0 + 1 == h ? 0 : j0 + 1;
    const uint8_t* t00 = t->px + 4 * ((size_t)j0 * t->w + i0);
    const uint8_t* t10 = t->px + 4 * ((size_t)j0 * t->w + i1);
    const uint8_t* t01 = t->px + 4 * ((size_t)j1 * t->w + i0);
    const uint8_t* t11 = t->px + 4 * ((size_t)j1 * t->w + i1);
    const float k = 1.0f / 255.0f;
    const float w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b;
    for (int c = 0; c < 4; ++c)
        rgba[c] = w00 * ((float)t00[c] * k) + w10 * ((float)t10[c] * k) + w01 * ((float)t01[c] * k) + w11 * ((float)t11[c] * k);
}

static int trace(const oracle_whitted_scene* s, w3 o, w3 d, float tmin, float tmax, int any, int* tri, float* t, float* u, float* v)
{
    const float O[3] = { o.x, o.y, o.z }, D[3] = { d.x, d.y, d.z };
    int best = -1;
    float bt = tmax, bu = 0.0f, bv = 0.0f;
    for (uint32_t i = 0; i < s->n_triangles; ++i) {
        float tt, uu, vv;
        const uint32_t* ix = s->indices + 3 * i;
        if (oracle_tri_intersect(s->positions + 3 * ix[0], s->positions + 3 * ix[1], s->positions + 3 * ix[2], O, D, tmin, tmax, &tt, &uu, &vv) && tt < bt) {
            bt = tt;
            bu = uu;
            bv = vv;
            best = (int)i;
            if (any) break;
        }
    }
    *tri = best;
    *t = bt;
    *u = bu;
    *v = bv;
    return best >= 0;
}

/* whitted.cu:49-80 */
static w3 schlick(w3 spec, float VdotH)
{
    const float k = powf(1.0f - VdotH, 5.0f);
    return wadd(spec, wscale(wsub(W3(1.0f, 1.0f, 1.0f), spec), k));
}
static float vis(float NdotL, float NdotV, float alpha)
{
    const float a2 = alpha * alpha;
    const float g0 = NdotL * sqrtf(NdotV * NdotV * (1.0f - a2) + a2);
    const float g1 = NdotV * sqrtf(NdotL * NdotL * (1.0f - a2) + a2);
    return 2.0f * NdotL * NdotV / (g0 + g1);
}
static float ggx_normal(float NdotH, float alpha)
{
    const float a2 = alpha * alpha;
    const float n2 = NdotH * NdotH;
    const float x = n2 * (a2 - 1.0f) + 1.0f;
    return a2 / (3.14159265358979323846f * x * x);
}

/* What the closest-hit program reads of a hit, either kind of scene (getLocalGeometry, LocalGeometry.h:55-141): P and N in world space,
   the triangle's corners in the space dp/du, dp/dv are taken in (object space: :118-134), its texture coordinates and its material. */
typedef struct {
    w3 P, N;
    w3 P0, P1, P2;
    float UV0[2], UV1[2], UV2[2], UV[2];
    uint32_t material;
} hit_geom;

/* UV (LocalGeometry.h:88-102): interpolated, or the barycentrics when the mesh has none */
static void hit_uv(hit_geom* g, const float* texcoords, const uint32_t* ix, float w0, float bu, float bv)
{
    g->UV0[0] = 0.0f; g->UV0[1] = 0.0f;
    g->UV1[0] = 0.0f; g->UV1[1] = 1.0f;
    g->UV2[0] = 1.0f; g->UV2[1] = 0.0f;
    g->UV[0] = bu; g->UV[1] = bv;
    if (texcoords) {
        for (int k = 0; k < 2; ++k) {
            g->UV0[k] = texcoords[2 * ix[0] + k];
            g->UV1[k] = texcoords[2 * ix[1] + k];
            g->UV2[k] = texcoords[2 * ix[2] + k];
            g->UV[k] = w0 * g->UV0[k] + bu * g->UV1[k] + bv * g->UV2[k];
        }
    }
}

/* the pipeline both kinds of scene share: raygen, closest hit + shading, occlusion, miss, accumulation, make_color.  `closest` traces a
   radiance ray and fills hit_geom; `occluded` is the any-hit occlusion ray. */
typedef struct {
    const void* scene;
    int (*closest)(const void* scene, w3 o, w3 d, hit_geom* g);
    int (*occluded)(const void* scene, w3 o, w3 d, float tmin, float tmax);
    const oracle_pbr* materials;
    const oracle_mat_tex* mat_tex;
    const oracle_point_light* lights;
    uint32_t n_lights;
    const float *eye, *U, *V, *W, *miss;
} pipeline;

/* __closesthit__radiance (whitted.cu:255-337) after getLocalGeometry */
static w3 shade(const pipeline* pl, const hit_geom* g, w3 rd, uint64_t* n_rays, uint64_t* n_occl)
{
    const w3 P = g->P;
    w3 N = g->N;
    const uint32_t mi = g->material;
    const oracle_pbr* m = pl->materials + mi;
    w3 base = W3(m->base_color[0], m->base_color[1], m->base_color[2]);
    float mr_y = 1.0f, mr_z = 1.0f; /* the (1,1,1,1) of an absent metallic-roughness texture, whitted.cu:271 */
    if (pl->mat_tex) {
        const oracle_mat_tex* mt = pl->mat_tex + mi;
        float tc[4];
        if (mt->base_color.px) { /* base_color *= linearize( tex2D ), whitted.cu:78-85, 264-267 */
            oracle_tex2d(&mt->base_color, g->UV[0], g->UV[1], tc);
            base = wmul(base, W3(powf(tc[0], 2.2f), powf(tc[1], 2.2f), powf(tc[2], 2.2f)));
        }
        if (mt->metallic_roughness.px) { /* (occlusion, roughness, metallic), :272-276 */
            oracle_tex2d(&mt->metallic_roughness, g->UV[0], g->UV[1], tc);
            mr_y = tc[1];
            mr_z = tc[2];
        }
        if (mt->normal.px) { /* whitted.cu:288-292 over LocalGeometry.h:118-134 (dp/du, dp/dv in object space) */
            const float du1 = g->UV0[0] - g->UV2[0], du2 = g->UV1[0] - g->UV2[0], dv1 = g->UV0[1] - g->UV2[1], dv2 = g->UV1[1] - g->UV2[1];
            const w3 dp1 = wsub(g->P0, g->P2), dp2 = wsub(g->P1, g->P2);
            const float det = du1 * dv2 - dv1 * du2;
            const float invdet = 1.0f / det;
            const w3 dpdu = wscale(wsub(wscale(dp1, dv2), wscale(dp2, dv1)), invdet);
            const w3 dpdv = wscale(wadd(wscale(dp1, -du2), wscale(dp2, du1)), invdet);
            oracle_tex2d(&mt->normal, g->UV[0], g->UV[1], tc);
            const float nx = 2.0f * tc[0] - 1.0f, ny = 2.0f * tc[1] - 1.0f, nz = 2.0f * tc[2] - 1.0f;
            N = wnormalize(wadd(wadd(wscale(wnormalize(dpdu), nx), wscale(wnormalize(dpdv), ny)), wscale(N, nz)));
        }
    }
    const float metallic = m->metallic * mr_z, roughness = m->roughness * mr_y; /* :269-276 */
    const float F0 = 0.04f;
    const w3 diff_color = wscale(wscale(base, 1.0f - F0), 1.0f - metallic);
    const w3 spec_color = wadd(W3(F0, F0, F0), wscale(wsub(base, W3(F0, F0, F0)), metallic)); /* lerp, vec_math.h:496-499 */
    const float alpha = roughness * roughness;
    w3 result = W3(0.0f, 0.0f, 0.0f);
    for (uint32_t l = 0; l < pl->n_lights; ++l) {
        const oracle_point_light* L = pl->lights + l;
        const w3 toL = wsub(W3(L->position[0], L->position[1], L->position[2]), P);
        const float Ldist = wlength(toL);
        const w3 Lv = wscale(toL, 1.0f / Ldist); /* float3 / float: vec_math.h:479-483 */
        const w3 Vv = wneg(wnormalize(rd));      /* the world ray direction (whitted.cu:307) */
        const w3 H = wnormalize(wadd(Lv, Vv));
        const float NdotL = wdot(N, Lv), NdotV = wdot(N, Vv), NdotH = wdot(N, H), VdotH = wdot(Vv, H);
        if (NdotL > 0.0f && NdotV > 0.0f) {
            *n_rays += 1;
            *n_occl += 1;
            if (!pl->occluded(pl->scene, P, Lv, 0.001f, Ldist - 0.001f)) {
                const w3 F = schlick(spec_color, VdotH);
                const float G = vis(NdotL, NdotV, alpha);
                const float D = ggx_normal(NdotH, alpha);
                const w3 diff = wscale(wmul(wsub(W3(1.0f, 1.0f, 1.0f), F), diff_color), 1.0f / 3.14159265358979323846f);
                const w3 spec = wscale(wscale(F, G), D);
                const w3 lc = wscale(W3(L->color[0], L->color[1], L->color[2]), L->intensity);
                result = wadd(result, wmul(wscale(lc, NdotL), wadd(diff, spec)));
            }
        }
    }
    return result;
}

/* one subframe: accum (float4 per pixel, read when subframe > 0) and image (uchar4) are updated in place; rays[0] += rays
   traced, rays[1] += occlusion rays among them */
static void render(const pipeline* pl, uint32_t width, uint32_t height, uint32_t subframe, float* accum, uint8_t* image, uint64_t* rays, int threads)
{
    uint64_t n_rays = 0, n_occl = 0;
    const w3 eye = wld(pl->eye, 0), U = wld(pl->U, 0), V = wld(pl->V, 0), Wv = wld(pl->W, 0);
    if (threads < 1) threads = 1;
#pragma omp parallel for schedule(dynamic, 4) num_threads(threads) reduction(+ : n_rays, n_occl)
    for (int64_t yy = 0; yy < (int64_t)height; ++yy)
        for (uint32_t x = 0; x < width; ++x) {
            const uint32_t y = (uint32_t)yy, idx = y * width + x;
            /* __raygen__pinhole, whitted.cu:183-240 */
            uint32_t seed = oracle_tea4(y * width + x, subframe);
            float jx = 0.0f, jy = 0.0f;
            if (subframe != 0) {
                jx = oracle_rnd(&seed) - 0.5f; /* x first: source order */
                jy = oracle_rnd(&seed) - 0.5f;
            }
            const float dx = 2.0f * (((float)x + jx) / (float)width) - 1.0f;
            const float dy = 2.0f * (((float)y + jy) / (float)height) - 1.0f;
            const w3 rd = wnormalize(wadd(wadd(wscale(U, dx), wscale(V, dy)), Wv));
            w3 result = wld(pl->miss, 0); /* __miss__constant_radiance */
            hit_geom g;
            n_rays += 1;
            if (pl->closest(pl->scene, eye, rd, &g)) result = shade(pl, &g, rd, &n_rays, &n_occl);
            /* whitted.cu:226-239 */
            w3 acc = result;
            if (subframe > 0) {
                const float a = 1.0f / (float)(subframe + 1);
                const w3 prev = W3(accum[4 * idx], accum[4 * idx + 1], accum[4 * idx + 2]);
                acc = wadd(prev, wscale(wsub(acc, prev), a));
            }
            accum[4 * idx + 0] = acc.x;
            accum[4 * idx + 1] = acc.y;
            accum[4 * idx + 2] = acc.z;
            accum[4 * idx + 3] = 1.0f;
            const float gm = (float)(1.0 / 2.2f); /* make_color, :164-173 */
            image[4 * idx + 0] = (uint8_t)(powf(wclamp(acc.x, 0.0f, 1.0f), gm) * 255.0f);
            image[4 * idx + 1] = (uint8_t)(powf(wclamp(acc.y, 0.0f, 1.0f), gm) * 255.0f);
            image[4 * idx + 2] = (uint8_t)(powf(wclamp(acc.z, 0.0f, 1.0f), gm) * 255.0f);
            image[4 * idx + 3] = 255u;
        }
    if (rays) {
        rays[0] += n_rays;
        rays[1] += n_occl;
    }
}

/* ---- one mesh in world space ---- */
static int mesh_closest(const void* scene, w3 o, w3 d, hit_geom* g)
{
    const oracle_whitted_scene* s = (const oracle_whitted_scene*)scene;
    int tri;
    float t, bu, bv;
    if (!trace(s, o, d, 0.01f, 1e16f, 0, &tri, &t, &bu, &bv)) return 0;
    /* getLocalGeometry (LocalGeometry.h:55-141), mesh in world space */
    const uint32_t* ix = s->indices + 3 * (uint32_t)tri;
    g->P0 = wld(s->positions, ix[0]);
    g->P1 = wld(s->positions, ix[1]);
    g->P2 = wld(s->positions, ix[2]);
    const float w0 = 1.0f - bu - bv;
    g->P = wadd(wadd(wscale(g->P0, w0), wscale(g->P1, bu)), wscale(g->P2, bv));
    g->N = wnormalize(wcross(wsub(g->P1, g->P0), wsub(g->P2, g->P0)));
    if (s->normals) {
        const w3 N0 = wld(s->normals, ix[0]), N1 = wld(s->normals, ix[1]), N2 = wld(s->normals, ix[2]);
        g->N = wnormalize(wadd(wadd(wscale(N0, w0), wscale(N1, bu)), wscale(N2, bv)));
    }
    hit_uv(g, s->texcoords, ix, w0, bu, bv);
    g->material = s->tri_material ? s->tri_material[tri] : 0u;
    return 1;
}
static int mesh_occluded(const void* scene, w3 o, w3 d, float tmin, float tmax)
{
    int tri;
    float t, u, v;
    return trace((const oracle_whitted_scene*)scene, o, d, tmin, tmax, 1, &tri, &t, &u, &v);
}

int oracle_whitted_render(const oracle_whitted_scene* s, uint32_t width, uint32_t height, uint32_t subframe, float* accum, uint8_t* image,
                          uint64_t* rays, int threads)
{
    if (!s || !accum || !image || width == 0 || height == 0 || s->n_triangles == 0) return -1;
    const pipeline pl = { s, mesh_closest, mesh_occluded, s->materials, s->mat_tex, s->lights, s->n_lights, s->eye, s->U, s->V, s->W, s->miss };
    render(&pl, width, height, subframe, accum, image, rays, threads);
    return 0;
}

/* ---- instanced meshes (sutil::Scene's two levels) ----
   W2O is the transform's inverse as the contract states it: adj(A) / det in double, the translation -B t in double, each entry rounded
   once to float.  A ray goes to object space through xform_point / xform_vector's operation order, not renormalised, so t is the same
   number in both spaces.  Brute force in instance order, then in the mesh's triangle order; a hit is kept only when t < best, which
   leaves the lowest (instance, triangle) on ties. */
typedef struct {
    const oracle_whitted_iscene* s;
    float* w2o;     /* 12 per instance */
    double* box;    /* 6 per mesh: the object-space bounds of its vertices, grown by the cull's margin */
} iprep;

static int inverse34(const float* tr, float* w2o)
{
    double A[3][4];
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 4; ++k) A[r][k] = tr[4 * r + k];
    const double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                       A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
    if (!isfinite(det) || fabs(det) < 1e-30) return -1;
    double B[3][4];
    B[0][0] = (A[1][1] * A[2][2] - A[1][2] * A[2][1]) / det;
    B[0][1] = (A[0][2] * A[2][1] - A[0][1] * A[2][2]) / det;
    B[0][2] = (A[0][1] * A[1][2] - A[0][2] * A[1][1]) / det;
    B[1][0] = (A[1][2] * A[2][0] - A[1][0] * A[2][2]) / det;
    B[1][1] = (A[0][0] * A[2][2] - A[0][2] * A[2][0]) / det;
    B[1][2] = (A[0][2] * A[1][0] - A[0][0] * A[1][2]) / det;
    B[2][0] = (A[1][0] * A[2][1] - A[1][1] * A[2][0]) / det;
    B[2][1] = (A[0][1] * A[2][0] - A[0][0] * A[2][1]) / det;
    B[2][2] = (A[0][0] * A[1][1] - A[0][1] * A[1][0]) / det;
    for (int r = 0; r < 3; ++r) B[r][3] = -(B[r][0] * A[0][3] + B[r][1] * A[1][3] + B[r][2] * A[2][3]);
    for (int k = 0; k < 12; ++k) {
        w2o[k] = (float)B[k / 4][k % 4];
        if (!isfinite(w2o[k])) return -1;
    }
    return 0;
}

/* M (p, 1), M (d, 0) and M^T n for a row-major 3x4 M: one rounding per operation, in row order */
static w3 xf_point(const float* m, w3 p)
{
    return W3(m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3], m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7], m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11]);
}
static w3 xf_vector(const float* m, w3 d)
{
    return W3(m[0] * d.x + m[1] * d.y + m[2] * d.z, m[4] * d.x + m[5] * d.y + m[6] * d.z, m[8] * d.x + m[9] * d.y + m[10] * d.z);
}
static w3 xf_normal(const float* m, w3 n)
{
    return W3(m[0] * n.x + m[4] * n.y + m[8] * n.z, m[1] * n.x + m[5] * n.y + m[9] * n.z, m[2] * n.x + m[6] * n.y + m[10] * n.z);
}

static void iprep_free(iprep* p)
{
    free(p->w2o);
    free(p->box);
    p->w2o = NULL;
    p->box = NULL;
}

static int iprep_make(const oracle_whitted_iscene* s, iprep* p)
{
    p->s = s;
    p->w2o = NULL;
    p->box = NULL;
    if (!s || !s->meshes || !s->instances || !s->materials || s->n_meshes == 0 || s->n_instances == 0) return -1;
    p->w2o = (float*)malloc(sizeof(float) * 12 * s->n_instances);
    p->box = (double*)malloc(sizeof(double) * 6 * s->n_meshes);
    if (!p->w2o || !p->box) {
        iprep_free(p);
        return -1;
    }
    for (uint32_t k = 0; k < s->n_meshes; ++k) {
        const oracle_whitted_mesh* m = s->meshes + k;
        double lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
        for (uint32_t i = 0; i < m->n_vertices; ++i)
            for (int a = 0; a < 3; ++a) {
                lo[a] = fmin(lo[a], m->positions[3 * i + a]);
                hi[a] = fmax(hi[a], m->positions[3 * i + a]);
            }
        /* the cull's margin: 1e-3 of the box's extent plus 1e-3 of its distance from the object's origin -- three orders of magnitude
           above what float32 Moeller-Trumbore can place a hit outside its triangle */
        double ext = 0.0, far = 0.0;
        for (int a = 0; a < 3; ++a) {
            ext = fmax(ext, hi[a] - lo[a]);
            far = fmax(far, fmax(fabs(lo[a]), fabs(hi[a])));
        }
        const double margin = 1e-3 * (ext + far) + 1e-30;
        for (int a = 0; a < 3; ++a) {
            p->box[6 * k + a] = lo[a] - margin;
            p->box[6 * k + 3 + a] = hi[a] + margin;
        }
        for (uint32_t i = 0; i < 3 * m->n_triangles; ++i)
            if (m->indices[i] >= m->n_vertices) {
                iprep_free(p);
                return -1;
            }
    }
    for (uint32_t i = 0; i < s->n_instances; ++i) {
        const oracle_whitted_instance* q = s->instances + i;
        if (q->mesh >= s->n_meshes || inverse34(q->transform, p->w2o + 12 * i) != 0) {
            iprep_free(p);
            return -1;
        }
        const oracle_whitted_mesh* m = s->meshes + q->mesh;
        for (uint32_t t = 0; t < m->n_triangles; ++t)
            if ((uint64_t)q->material_offset + (m->tri_material ? m->tri_material[t] : 0u) >= s->n_materials) {
                iprep_free(p);
                return -1;
            }
    }
    return 0;
}

/* whether the line o + t d, t >= tmin - 1, can meet the (grown) box: the slab test in double.  Only ever skips instances the triangle
   test could not hit (tests/test_oracle_whitted.py holds the frames with the cull on and off bitwise equal). */
static int line_meets_box(const double* b, w3 o, w3 d, float tmin)
{
    double a = (double)tmin - 1.0, z = INFINITY;
    const double O[3] = { o.x, o.y, o.z }, D[3] = { d.x, d.y, d.z };
    for (int k = 0; k < 3; ++k) {
        if (D[k] == 0.0) {
            if (O[k] < b[k] || O[k] > b[3 + k]) return 0;
            continue;
        }
        const double t0 = (b[k] - O[k]) / D[k], t1 = (b[3 + k] - O[k]) / D[k];
        a = fmax(a, fmin(t0, t1));
        z = fmin(z, fmax(t0, t1));
    }
    return a <= z;
}

static int itrace(const iprep* p, w3 o, w3 d, float tmin, float tmax, int any, int* inst, int* tri, float* t, float* u, float* v)
{
    const oracle_whitted_iscene* s = p->s;
    int bi = -1, btri = -1;
    float bt = tmax, bu = 0.0f, bv = 0.0f;
    for (uint32_t i = 0; i < s->n_instances && !(any && bi >= 0); ++i) {
        const oracle_whitted_instance* q = s->instances + i;
        const oracle_whitted_mesh* m = s->meshes + q->mesh;
        const float* w2o = p->w2o + 12 * i;
        const w3 oo = xf_point(w2o, o), od = xf_vector(w2o, d);
        if (s->cull && !line_meets_box(p->box + 6 * q->mesh, oo, od, tmin)) continue;
        const float O[3] = { oo.x, oo.y, oo.z }, D[3] = { od.x, od.y, od.z };
        for (uint32_t k = 0; k < m->n_triangles; ++k) {
            float tt, uu, vv;
            const uint32_t* ix = m->indices + 3 * k;
            if (oracle_tri_intersect(m->positions + 3 * ix[0], m->positions + 3 * ix[1], m->positions + 3 * ix[2], O, D, tmin, tmax, &tt, &uu, &vv) && tt < bt) {
                bt = tt;
                bu = uu;
                bv = vv;
                bi = (int)i;
                btri = (int)k;
                if (any) break;
            }
        }
    }
    *inst = bi;
    *tri = btri;
    *t = bt;
    *u = bu;
    *v = bv;
    return bi >= 0;
}

static int inst_closest(const void* scene, w3 o, w3 d, hit_geom* g)
{
    const iprep* p = (const iprep*)scene;
    int ii, tri;
    float t, bu, bv;
    if (!itrace(p, o, d, 0.01f, 1e16f, 0, &ii, &tri, &t, &bu, &bv)) return 0;
    /* getLocalGeometry of an instanced mesh: P through O2W (LocalGeometry.h:84), Ng = W2O^T normalize(cross) not renormalised (:103) and
       N = Ng without vertex normals (:116), N = normalize(W2O^T interp(N)) with them (:112); dp/du, dp/dv stay in object space */
    const oracle_whitted_instance* q = p->s->instances + ii;
    const oracle_whitted_mesh* m = p->s->meshes + q->mesh;
    const float* w2o = p->w2o + 12 * ii;
    const uint32_t* ix = m->indices + 3 * (uint32_t)tri;
    g->P0 = wld(m->positions, ix[0]);
    g->P1 = wld(m->positions, ix[1]);
    g->P2 = wld(m->positions, ix[2]);
    const float w0 = 1.0f - bu - bv;
    g->P = xf_point(q->transform, wadd(wadd(wscale(g->P0, w0), wscale(g->P1, bu)), wscale(g->P2, bv)));
    g->N = xf_normal(w2o, wnormalize(wcross(wsub(g->P1, g->P0), wsub(g->P2, g->P0))));
    if (m->normals) {
        const w3 N0 = wld(m->normals, ix[0]), N1 = wld(m->normals, ix[1]), N2 = wld(m->normals, ix[2]);
        g->N = wnormalize(xf_normal(w2o, wadd(wadd(wscale(N0, w0), wscale(N1, bu)), wscale(N2, bv))));
    }
    hit_uv(g, m->texcoords, ix, w0, bu, bv);
    g->material = q->material_offset + (m->tri_material ? m->tri_material[tri] : 0u);
    return 1;
}
static int inst_occluded(const void* scene, w3 o, w3 d, float tmin, float tmax)
{
    int ii, tri;
    float t, u, v;
    return itrace((const iprep*)scene, o, d, tmin, tmax, 1, &ii, &tri, &t, &u, &v);
}

int oracle_whitted_render_instanced(const oracle_whitted_iscene* s, uint32_t width, uint32_t height, uint32_t subframe, float* accum, uint8_t* image,
                                    uint64_t* rays, int threads)
{
    if (!s || !accum || !image || width == 0 || height == 0) return -1;
    iprep p;
    if (iprep_make(s, &p) != 0) return -1;
    const pipeline pl = { &p, inst_closest, inst_occluded, s->materials, s->mat_tex, s->lights, s->n_lights, s->eye, s->U, s->V, s->W, s->miss };
    render(&pl, width, height, subframe, accum, image, rays, threads);
    iprep_free(&p);
    return 0;
}

int oracle_whitted_trace_instanced(const oracle_whitted_iscene* s, const float* o, const float* d, float tmin, float tmax, int* instance, int* triangle,
                                   float* t, float* u, float* v)
{
    iprep p;
    if (!o || !d || !instance || !triangle || !t || !u || !v || iprep_make(s, &p) != 0) return -1;
    const int hit = itrace(&p, wld(o, 0), wld(d, 0), tmin, tmax, 0, instance, triangle, t, u, v);
    iprep_free(&p);
    return hit;
}

/* ---- the closest-hit program alone ----
   shade() on a hit the caller states: world P and N, the triangle's corners (the space dp/du, dp/dv are taken in) and their texture
   coordinates, UV, the world ray direction, one material with its optional textures, the lights.  Occlusion rays meet the triangle of
   the three corners alone, or nothing when no_occlusion is set. */
static int point_occluded(const void* scene, w3 o, w3 d, float tmin, float tmax)
{
    const float* c = (const float*)scene;
    const float O[3] = { o.x, o.y, o.z }, D[3] = { d.x, d.y, d.z };
    float t, u, v;
    return oracle_tri_intersect(c, c + 3, c + 6, O, D, tmin, tmax, &t, &u, &v);
}
static int point_unoccluded(const void* scene, w3 o, w3 d, float tmin, float tmax)
{
    (void)scene; (void)o; (void)d; (void)tmin; (void)tmax;
    return 0;
}

int oracle_whitted_shade_point(const float* P, const float* N, const float* corners, const float* corner_uv, const float* UV, const float* rd,
                               const oracle_pbr* material, const oracle_mat_tex* textures, const oracle_point_light* lights, uint32_t n_lights,
                               int no_occlusion, float* rgb)
{
    if (!P || !N || !corners || !corner_uv || !UV || !rd || !material || !rgb || (n_lights && !lights)) return -1;
    hit_geom g;
    g.P = wld(P, 0);
    g.N = wld(N, 0);
    g.P0 = wld(corners, 0);
    g.P1 = wld(corners, 1);
    g.P2 = wld(corners, 2);
    for (int k = 0; k < 2; ++k) {
        g.UV0[k] = corner_uv[k];
        g.UV1[k] = corner_uv[2 + k];
        g.UV2[k] = corner_uv[4 + k];
        g.UV[k] = UV[k];
    }
    g.material = 0u;
    const pipeline pl = { corners, NULL, no_occlusion ? point_unoccluded : point_occluded, material, textures, lights, n_lights, NULL, NULL, NULL, NULL, NULL };
    uint64_t n_rays = 0, n_occl = 0;
    const w3 c = shade(&pl, &g, wld(rd, 0), &n_rays, &n_occl);
    rgb[0] = c.x;
    rgb[1] = c.y;
    rgb[2] = c.z;
    return (int)n_occl;
}
