// rtgo_ray_shade.inc -- the shading half of one ray of one lane's path: the state machine that replaces the recursion of
// __closesthit__ch / __miss__ms / __closesthit__full_occlusion (kernel.cu:419-549), from the `hit` and `h` rtgo_ray_trace.inc left
// (the streaming loop may run it later than the trace, for several lanes at once).  A textual fragment, not a function: it works on the
// per-sample state of the enclosing scope -- active, depth, phase, seed, ro, rd, tmin, tmax, result (FOLDLATE: ended_in), any_hit, lvA /
// lvPrim (or the LDS records s_lv), sN, sRr, sDist, sPrim, sLight -- which has to stay in registers (a lambda capturing the level arrays
// by reference put them in scratch).
                bool done = false;       // path ended: `term` is the payload of the ray at level `depth`
                v3 term = mk(0, 0, 0);
                int ends_in = kEndsInZero;   // FOLDLATE: which payload that is

                if (PATH) {
                    if (!hit) {
                        term = p.bg;  // __miss__ms, kernel.cu:419-423
                        ends_in = kEndsInBackground;
                        done = true;
                    } else {
                        // __closesthit__ch, path branch: kernel.cu:426-475
                        const float4 m3 = s_mat[MS * h.prim + 0], m5 = s_mat[MS * h.prim + 2];
                        // scenes of flat primitives only (cornell, checkered): N and the sampling tangent come from the frame build_kernel
                        // computed (the same bits); scenes with quadrics keep the per-hit computation (a per-lane choice cost more than it saved)
                        v3 N, Xf = mk(0.0f, 0.0f, 0.0f);
                        if constexpr (FRAMES) {
                            const float4 f0 = s_frame[2 * h.prim + 0], f1 = s_frame[2 * h.prim + 1];
                            N = mk(f0.x, f0.y, f0.z);
                            Xf = mk(f1.x, f1.y, f1.z);
                        } else {
                            N = vnormalize(h.n);
                        }
                        const float t = h.t;
                        const float rayEpsilon = 1e-6f * fmaxf(t * t, 1.0f);
                        // (kernel.cu:439 normalises the ray direction again; every direction this kernel traces is a unit vector already --
                        // raygen's normalize, GetRayOnHemisphere's orthonormal combination -- so that is an ulp, inside the stated tolerance)
#ifdef RTGO_LITERAL_SHADING
                        const v3 x = vadd(ro, vscale(vnormalize(rd), t));
#else
                        const v3 x = vadd(ro, vscale(rd, t));
#endif
                        if (faces_away(N, vsub(ro, x))) {
                            N = vscale(N, -1.0f);
                            Xf = vscale(Xf, -1.0f);
                        }
                        if (m5.x > 0.01f) {
                            term = mk(m5.x, m5.y, m5.z);
                            ends_in = h.prim;
                            done = true;
                        } else if (depth < p.max_depth) {
                            const v3 Ra = hemisphere<true>(N, N, 0.0f, seed, FRAMES, Xf);
                            const v3 wk = vadd(mk(0.0f, 0.0f, 0.0f), vscale(mk(m3.x, m3.y, m3.z), vdot(N, Ra)));
                            if constexpr (UNIT16) {
                                float* lv = s_lv + depth * (LVW * 256);   // (bshift is 8: one address, the three words at fixed offsets)
                                lv[0] = wk.x;
                                lv[256] = wk.y;
                                lv[512] = wk.z;
                            } else if constexpr (LVLDS) {
                                s_lv[(depth * LVW + 0) << bshift] = wk.x;
                                s_lv[(depth * LVW + 1) << bshift] = wk.y;
                                s_lv[(depth * LVW + 2) << bshift] = wk.z;
                            } else {
#pragma unroll
                                for (int k = 0; k < kMaxLevels; ++k)
                                    if (k == depth) lvA[k] = wk;
                            }
                            ++depth;
                            ro = x;
                            rd = Ra;
                            tmin = rayEpsilon;
                            tmax = 1e6f;
                        } else {
                            term = mk(0.0f, 0.0f, 0.0f);
                            done = true;
                        }
                    }
                } else {
                    if (phase == 1) {
                        // back from the shadow ray: kernel.cu:498-535 (+ __closesthit__full_occlusion :539-549)
                        c_occl += 1;
                        v3 illum = mk(1.0f, 1.0f, 1.0f);  // occlusion miss leaves the payload untouched (SURVEY Q2)
                        if (hit) {
                            const float4 b5 = s_mat[MS * h.prim + 2];
                            illum = mk(fminf(b5.x, 1.0f), fminf(b5.y, 1.0f), fminf(b5.z, 1.0f));
                        }
                        const LightRec& L = s_lights[sLight];
                        const float4 m3 = s_mat[MS * sPrim + 0];
                        const v3 kd = mk(m3.x, m3.y, m3.z);
                        const float spec = m3.w;
                        const v3 Lm = rd;
                        const v3 lightNormal = mk(L.normal[0], L.normal[1], L.normal[2]);
                        const v3 lightColor = vscale(illum, fabsf(vdot(Lm, lightNormal)));
                        const float falloff = div_cr(1.0f, 1.0f + L.falloff * sDist);
                        const v3 compDiffuse =
                            vmul(vscale(lightColor, fmaxf(vdot(sN, Lm), 0.0f)), kd);   // (kernel.cu:503 tests dot(N, V) < 0 again: after the flip it never is)
                        const v3 a = vadd(mk(0.0f, 0.0f, 0.0f), vscale(compDiffuse, falloff));
                        bool bounce = false;
                        v3 r = mk(0, 0, 0);
                        if (depth < p.max_depth) {
                            if (p.ambient) {
                                if (spec > 0.5f) {
                                    r = hemisphere<false>(sN, sRr, spec, seed);
                                    bounce = true;
                                }
                            } else {
                                r = spec < 0.5f ? hemisphere<false>(sN, sN, 0.0f, seed) : hemisphere<false>(sN, sRr, spec, seed);
                                bounce = true;
                            }
                        }
                        if (bounce) {
                            if constexpr (LVLDS) {
                                s_lv[(depth * LVW + 0) << bshift] = a.x;
                                s_lv[(depth * LVW + 1) << bshift] = a.y;
                                s_lv[(depth * LVW + 2) << bshift] = a.z;
                                s_lv[(depth * LVW + 3) << bshift] = __int_as_float(sPrim);
                            } else {
#pragma unroll
                                for (int k = 0; k < kMaxLevels; ++k)
                                    if (k == depth) {
                                        lvA[k] = a;
                                        lvPrim[k] = sPrim;
                                    }
                            }
                            ++depth;
                            rd = r;            // ro = x and tmin = rayEpsilon are still those of the shadow ray
                            tmax = 1e6f;
                            phase = 0;
                        } else {
                            term = a;
                            if (p.ambient && depth < p.max_depth) term = vadd(term, vmul(kd, mk(0.1f, 0.1f, 0.1f)));
                            done = true;
                        }
                    } else if (!hit) {
                        term = p.bg;
                        done = true;
                    } else {
                        // __closesthit__ch, distributed branch up to the shadow trace: kernel.cu:426-455, 477-499
                        const float4 m5 = s_mat[MS * h.prim + 2];
                        v3 N = vnormalize(h.n);
                        const float t = h.t;
                        const float rayEpsilon = 1e-6f * fmaxf(t * t, 1.0f);
                        const v3 dn = vnormalize(rd);   // (kept literal in distributed mode: see hemisphere())
                        const v3 x = vadd(ro, vscale(dn, t));
                        if (faces_away(N, vsub(ro, x))) N = vscale(N, -1.0f);
                        if (vlength(mk(m5.x, m5.y, m5.z)) > 0.01f) {
                            term = mk(1.0f, 1.0f, 1.0f);
                            done = true;
                        } else {
                            const int l = (int)(rnd(seed) * (float)(p.n_lights - 1));
                            const LightRec& L = s_lights[l];
                            const float ra = rnd(seed);  // Q1: v1 factor first
                            const float rb = rnd(seed);
                            const v3 samplingPos =
                                vadd(vadd(mk(L.corner[0], L.corner[1], L.corner[2]), vscale(mk(L.v1[0], L.v1[1], L.v1[2]), ra)),
                                     vscale(mk(L.v2[0], L.v2[1], L.v2[2]), rb));
                            const v3 toL = vsub(samplingPos, x);
                            const v3 Lm = vnormalize(toL);
                            const float lightDistance = vlength(toL);
                            const v3 omega = vneg(dn);
                            sRr = vadd(vneg(omega), vscale(N, 2.0f * vdot(N, omega)));
                            sN = N;
                            sDist = lightDistance;
                            sPrim = h.prim;
                            sLight = l;
                            ro = x;
                            rd = Lm;
                            tmin = rayEpsilon;
                            tmax = lightDistance - rayEpsilon;
                            phase = 1;
                        }
                    }
                }

                if (done) {
                    // fold the level records innermost-first: kernel.cu:471-472 (path), :504,519,531 (distributed)
                    if constexpr (FOLDLATE) {
                        // (the pair kernels' lock-step loop looks the payload up and folds after the loop, all lanes together: rtgo_render_body.inc)
                        ended_in = ends_in;
                    } else if constexpr (LVLDS) {
                        for (int k = depth - 1; k >= 0; --k) {
                            const v3 a = mk(s_lv[(k * LVW + 0) << bshift], s_lv[(k * LVW + 1) << bshift], s_lv[(k * LVW + 2) << bshift]);
                            if (PATH) {
                                term = vmul(a, term);
                            } else {
                                const int prim = __float_as_int(s_lv[(k * LVW + 3) << bshift]);
                                const float4 m3 = s_mat[MS * prim + 0], m4 = s_mat[MS * prim + 1];
                                term = vadd(a, vmul(mk(m4.x, m4.y, m4.z), term));
                                if (p.ambient) term = vadd(term, vmul(mk(m3.x, m3.y, m3.z), mk(0.1f, 0.1f, 0.1f)));
                            }
                        }
                    } else {
#pragma unroll
                        for (int k = kMaxLevels - 1; k >= 0; --k) {
                            if (k < depth) {
                                if (PATH) {
                                    term = vmul(lvA[k], term);
                                } else {
                                    const float4 m3 = s_mat[MS * lvPrim[k] + 0], m4 = s_mat[MS * lvPrim[k] + 1];
                                    term = vadd(lvA[k], vmul(mk(m4.x, m4.y, m4.z), term));
                                    if (p.ambient) term = vadd(term, vmul(mk(m3.x, m3.y, m3.z), mk(0.1f, 0.1f, 0.1f)));
                                }
                            }
                        }
                    }
                    if constexpr (!FOLDLATE) result = term;
                    active = false;
                }
