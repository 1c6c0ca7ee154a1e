// rtgo_ray_trace.inc -- the trace half of one ray of one lane's path (see rtgo_ray_shade.inc for the other half): the closest hit of
// (ro, rd, tmin, tmax) through the walk this instantiation uses, into `hit` and `h`, which it declares.  A textual fragment: it
// works on the per-sample state of the enclosing scope.  Included by the lock-step pass loop and by the streaming loop (rtgo_device.h).
                Hit h;
                c_rays += 1;
                bool hit;
                if constexpr (STATS) hit = closest_hit<COUNT>(s_nodes, s_prims, s_stack, bshift, ro, rd, tmin, tmax, h, c_nodes, c_tests);
                else if constexpr (PAIR)   // (what the launch vouches for is a constant, and its three words are LaunchParams::pair's)
                    hit = closest_hit_fast<false, LASTRAY, true, MASKS, SLAB, ROOMW>(s_nodes, s_prims, g_fprims, GridParams(), s_stack4, bshift, kPairSmall, p.pair.n_prims, 0, kCubRoom, p.pair.cub_mu, false,
                                                                        ro, rd, tmin, tmax, h, c_nodes, c_tests, LASTRAY ? Pred<MASKS>::ieq(depth, p.pair.last_depth) : Pred<MASKS>::off(), tl, ROOMW ? &p.pair : nullptr);
                else hit = closest_hit_fast<GRID, LASTRAY, PAIR, false>(s_nodes, s_prims, g_fprims, p.grid,
                                            s_stack4, bshift, p.n_small, p.n_prims, p.n_big_pairs, p.list_cub, p.cub_mu, p.tree_spheres != 0, ro, rd, tmin, tmax, h, c_nodes, c_tests,
                                            LASTRAY && depth == p.max_depth && p.emit_n != 0, tl, nullptr);
                if (COUNT && hit) c_hits += 1;
                any_hit = any_hit || hit;
                if constexpr (STATS) CmpWalk::check(p, s_stack, bshift, ro, rd, tmin, tmax, hit, h, depth, phase);   // (diagnostic build: the fast walk on the same ray)

