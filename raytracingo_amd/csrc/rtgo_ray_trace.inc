// rtgo_ray_trace.inc -- the trace half of one ray of one lane's path (see rtgo_ray_shade.inc for the other half): the closest hit of
// (ro, rd, tmin, tmax) through the walk this instantiation uses, into `hit` and `h`, which it declares.  A textual fragment: it
// works on the per-sample state of the enclosing scope.  Included by the lock-step pass loop and by the streaming loop (rtgo_device.h).
                Hit h;
                c_rays += 1;
                bool hit;
                if constexpr (STATS) hit = closest_hit<COUNT>(s_nodes, s_prims, s_stack, bshift, ro, rd, tmin, tmax, h, c_nodes, c_tests);
                else hit = closest_hit_fast<GRID, LASTRAY>(s_nodes, s_prims, g_fprims, p.grid,
                                            s_stack4, bshift, p.n_small, p.n_prims, p.n_big_pairs, p.list_cub, p.cub_mu, p.tree_spheres != 0, ro, rd, tmin, tmax, h, c_nodes, c_tests,
                                            LASTRAY && depth == p.max_depth && p.emit_n != 0
#ifdef RTGO_TIMELINE
                                            , tl_big, tl_tree
#endif
                );
                if (COUNT && hit) c_hits += 1;
                any_hit = any_hit || hit;
#ifdef RTGO_CMPWALK
                if constexpr (STATS) {
                    // diagnostic build (tools/cmp_walks.py): the fast walk on the same ray, straight from global memory
                    Hit hf;
                    unsigned int d0 = 0, d1 = 0;
                    // (this lane's canonical stack is idle here: its own 8-byte slots serve as the fast walk's one-word entries)
                    // (RTGO_TREE=2 hands this launch the grid in p.fnodes: p.grid.n_cells > 0 then)
                    const bool hitf = p.grid.n_cells > 0
                        ? closest_hit_fast<true>(p.fnodes, p.fprims, p.fprims, p.grid, reinterpret_cast<unsigned int*>(s_stack), bshift + 1, p.n_small, p.n_prims, p.n_big_pairs, p.list_cub, p.cub_mu, p.tree_spheres != 0, ro, rd, tmin, tmax, hf, d0, d1, false)
                        : closest_hit_fast<false>(p.fnodes, p.fprims, p.fprims, p.grid, reinterpret_cast<unsigned int*>(s_stack), bshift + 1, p.n_small, p.n_prims, p.n_big_pairs, p.list_cub, p.cub_mu, p.tree_spheres != 0, ro, rd, tmin, tmax, hf, d0, d1, false);
                    const bool same = hit == hitf && (!hit || (h.t == hf.t && h.prim == hf.prim && h.n.x == hf.n.x && h.n.y == hf.n.y && h.n.z == hf.n.z));
                    if (!same) {
                        const unsigned int slot = atomicAdd(reinterpret_cast<unsigned int*>(p.cmp), 1u);
                        if (slot < 255u) {
                            float* r = p.cmp + 16 * (slot + 1);
                            r[0] = ro.x; r[1] = ro.y; r[2] = ro.z; r[3] = rd.x; r[4] = rd.y; r[5] = rd.z; r[6] = tmin; r[7] = tmax;
                            r[8] = hit ? h.t : -1.0f; r[9] = hit ? (float)h.prim : -1.0f; r[10] = hitf ? hf.t : -1.0f; r[11] = hitf ? (float)hf.prim : -1.0f;
                            r[12] = (float)depth; r[13] = (float)phase; r[14] = 0.0f; r[15] = 0.0f;
                        }
                    }
                }
#endif

