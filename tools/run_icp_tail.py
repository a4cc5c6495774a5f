#!/usr/bin/env python3
"""The tail of an ICP iteration (sums -> solve -> move -> seeds): the fused sums + move launch (tune icp_fused_sums 1 / 2) and the chain whose NEXT SEARCH
moves the cloud (tune icp_move_in_search 1 / 2) or also reduces the sums and solves first (tune icp_solve_in_search 1 / 2).
usage: run_icp_tail.py trace [n]            two 20-iteration exhaustive loops at n points, nothing else (under rocprofv3 --kernel-trace; tools/trace_iter.py)
       run_icp_tail.py ab [reps]            wall time per iteration, the arms alternating in ONE process — move in search / fused sums + move / three
                                            launches: 60 k / 120 k / 250 k exhaustive (20 iterations; 250 k is multi-slice: the first arm falls back to
                                            the second) and hw9's 4 000 points with the grid (800 iterations); median and spread (max - min) over reps;
                                            at 120 k also 256-thread workgroups (icp_fused_sums_threads); at every exhaustive size the six geometries
                                            of the sums + solve launch (icp_sums_solve_threads 256 / 512 x icp_sums_solve_pairs 1 / 2 / 4);
                                            at every exhaustive size the default geometry with the state snapshots copied on the stream / written by the
                                            kernel (icp_host_snapshots 2 / 1) x one arrival counter / one per replica (icp_ticket_levels 1 / 2);
                                            at every exhaustive size the chain sums -> search (icp_solve_in_search 1) with both snapshot forms
                                            and the six geometries of its sums launch (PCR_AB_SOLVE_ONLY=1: chain 4, these arms and the control alone)
       run_icp_tail.py stamps [n]           profile build (tools/ab_build.sh fsprof kabsch.hip -DPCR_FS_PROF; PCR_LIB_PATH=.../libpcr_fsprof.so): per workgroup
                                            the time from its row store to the end of its wait at the grid barrier, last iteration of a 20-iteration loop
       run_icp_tail.py ss_stamps [n] [T:P,...]   profile build (tools/ab_build.sh ssprof kabsch.hip -DPCR_SS_PROF; PCR_LIB_PATH=.../libpcr_ssprof.so): the sums +
                                            solve launch of the chain search -> sums + solve, last iteration of a 20-iteration loop, per geometry (threads :
                                            pairs) and per ticket form (icp_ticket_levels 1 / 2): per workgroup entry -> totals ready and totals ready ->
                                            ticket returned; for the last arriver ticket -> sums reduced -> solved -> published -> snapshot in host memory
                                            (the last launch of a call writes one unless icp_host_snapshots = 2)
       run_icp_tail.py sums_stamps [n] [T:P,...]   the same profile build: the sums launch of the chain sums -> search (icp_solve_in_search = 1), last iteration
                                            of a 20-iteration loop, per geometry: per workgroup entry -> totals ready and -> atomics performed
       run_icp_tail.py solve_stamps [n]     profile build (tools/ab_build.sh svprof nn1_brute.hip -DPCR_SV_PROF; PCR_LIB_PATH=.../libpcr_svprof.so): the prologue of
                                            the search that finishes an iteration, the solving wave of one workgroup, last search of a
                                            20-iteration loop: entry -> loads requested -> replicas in LDS -> solved -> barrier passed -> prologue done
PCR_TUNE="key=value,..." sets any other knob."""
import importlib, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
pcr = importlib.import_module("hands-on-point-cloud-processing_amd")
synth = importlib.import_module("hands-on-point-cloud-processing_amd.synth")
mode = sys.argv[1] if len(sys.argv) > 1 else "ab"
ctx = pcr.Context(0)
ctx.tune("icp_fused_sums_min", 1); ctx.tune("icp_fused_sums_grid", 1)      # every size and both searches take the fused launch when icp_fused_sums is 1
for kv in os.environ.get("PCR_TUNE", "").split(","):
    if "=" in kv:
        k_, v_ = kv.split("="); ctx.tune(k_, int(v_))


def pair(n):
    src, tgt = synth.kitti_like_pair(n)
    return ctx.cloud(src), ctx.cloud(tgt)


if mode == "trace":
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 120000
    cs, ct = pair(n); ctx.tune("nn_method", 1)
    for _ in range(2):
        T, st = ctx.icp_point2point(cs, ct, max_corr=1.0, max_iter=20, eps=0.0)
    print(f"n={n}: iters_run {st['iters_run']} last_pairs {st['last_pairs']}")
elif mode == "stamps":
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 120000
    cs, ct = pair(n); ctx.tune("nn_method", 1)
    ctx.icp_point2point(cs, ct, max_corr=1.0, max_iter=20, eps=0.0)
    ctx.tune("grid_stats", 1)
    for threads in (512, 256):
        ctx.tune("icp_fused_sums_threads", threads)
        ctx.icp_point2point(cs, ct, max_corr=1.0, max_iter=20, eps=0.0)
        w = ctx.nn1_stats(); k = max(w[14], 1)
        print(f"n={n} threads {threads}: workgroups stamped {w[14]}; row store -> end of wait: mean {w[12] / k / 100:.2f} us, longest {w[13] / 100:.2f} us; "
              f"kernel entry -> row store: mean {w[15] / k / 100:.2f} us")
elif mode == "ss_stamps":
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 120000
    geoms = [tuple(int(v) for v in g.split(":")) for g in (sys.argv[3] if len(sys.argv) > 3 else "512:4,512:2,512:1,256:4,256:2,256:1").split(",")]
    cs, ct = pair(n); ctx.tune("nn_method", 1); ctx.tune("icp_move_in_search", 1)
    ctx.icp_point2point(cs, ct, max_corr=1.0, max_iter=20, eps=0.0)
    ctx.tune("grid_stats", 1)
    for threads, pairs in geoms:
        ctx.tune("icp_sums_solve_threads", threads); ctx.tune("icp_sums_solve_pairs", pairs)
        for levels in (1, 2):
            ctx.tune("icp_ticket_levels", levels)
            for _ in range(3):
                ctx.icp_point2point(cs, ct, max_corr=1.0, max_iter=20, eps=0.0)
                w = ctx.nn1_stats(); k = max(w[14], 1)
                print(f"n={n} threads {threads} pairs {pairs} ticket levels {levels} chain {ctx.icp_last_chain()} snapshots {ctx.icp_last_snapshots()}: workgroups {w[14]}; "
                      f"entry -> totals ready: mean {w[12] / k / 100:.2f} us; "
                      f"totals ready -> ticket returned: mean {w[13] / k / 100:.2f} us, longest {w[15] / 100:.2f} us; last arriver: ticket -> sums reduced "
                      f"{w[0] / 100:.2f} us (acquired {w[2] / 100:.2f}, replicas in LDS {w[3] / 100:.2f}), -> solved {w[1] / 100:.2f} us, -> published {w[11] / 100:.2f} us, "
                      f"-> snapshot {w[4] / 100:.2f} us")
elif mode == "sums_stamps":
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 120000
    geoms = [tuple(int(v) for v in g.split(":")) for g in (sys.argv[3] if len(sys.argv) > 3 else "512:4,512:2,512:1,256:4,256:2,256:1").split(",")]
    cs, ct = pair(n); ctx.tune("nn_method", 1); ctx.tune("icp_solve_in_search", 1)
    ctx.icp_point2point(cs, ct, max_corr=1.0, max_iter=20, eps=0.0)
    ctx.tune("grid_stats", 1)
    for threads, pairs in geoms:
        ctx.tune("icp_sums_solve_threads", threads); ctx.tune("icp_sums_solve_pairs", pairs)
        for _ in range(3):
            ctx.icp_point2point(cs, ct, max_corr=1.0, max_iter=20, eps=0.0)
            w = ctx.nn1_stats(); k = max(w[14], 1)
            print(f"n={n} threads {threads} pairs {pairs} chain {ctx.icp_last_chain()}: workgroups {w[14]}; entry -> totals ready: mean {w[12] / k / 100:.2f} us; "
                  f"totals ready -> atomics performed: mean {w[13] / k / 100:.2f} us, longest {w[15] / 100:.2f} us")
elif mode == "solve_stamps":
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 120000
    cs, ct = pair(n); ctx.tune("nn_method", 1); ctx.tune("icp_solve_in_search", 1)
    ctx.icp_point2point(cs, ct, max_corr=1.0, max_iter=20, eps=0.0)
    ctx.tune("grid_stats", 1)
    for _ in range(5):
        ctx.icp_point2point(cs, ct, max_corr=1.0, max_iter=20, eps=0.0)
        w = ctx.nn1_stats()
        print(f"n={n} chain {ctx.icp_last_chain()}: the solving wave of workgroup 1, last search of the loop: entry -> loads requested {w[11] / 100:.2f} us, -> replicas in LDS "
              f"{w[12] / 100:.2f} us, -> solved {w[13] / 100:.2f} us, -> barrier passed {w[14] / 100:.2f} us, -> prologue done {w[15] / 100:.2f} us")
else:
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    # an arm: (icp_move_in_search, icp_fused_sums, icp_fused_sums_threads, icp_sums_solve_threads, icp_sums_solve_pairs, icp_host_snapshots, icp_ticket_levels,
    # icp_solve_in_search)
    KEYS = ("icp_move_in_search", "icp_fused_sums", "icp_fused_sums_threads", "icp_sums_solve_threads", "icp_sums_solve_pairs", "icp_host_snapshots", "icp_ticket_levels",
            "icp_solve_in_search")
    MV, FS, TL = (1, 1, 512, 0, 0, 0, 0, 2), (2, 1, 512, 0, 0, 0, 0, 2), (2, 2, 512, 0, 0, 0, 0, 2)
    GEO = tuple((1, 1, 512, t, p, 0, 0, 2) for t in (512, 256) for p in (4, 2, 1))
    SNAP = tuple((1, 1, 512, 0, 0, s_, l_, 2) for s_ in (2, 1) for l_ in (1, 2))
    SOLVE = tuple((1, 1, 512, 0, 0, s_, 0, 1) for s_ in (1, 2)) + tuple((1, 1, 512, t, p, 0, 0, 1) for t in (512, 256) for p in (4, 2, 1))
    GRID = (FS, TL)                               # (the control: the grid loop takes neither the move in the search nor what rides on it)
    CHAINS = (MV, FS, TL)
    if os.environ.get("PCR_AB_SNAP_ONLY"):        # (a short visit: the default chain and the four snapshot / ticket arms alone)
        GEO, CHAINS = (), (MV,)
    if os.environ.get("PCR_AB_SOLVE_ONLY"):       # (a short visit: chain 4, the arms of the chain sums -> search and the control)
        GEO, SNAP, CHAINS = (), (), (MV,)
    for n, method, iters, arms in ((60000, 1, 20, CHAINS + SNAP + GEO + SOLVE), (120000, 1, 20, CHAINS + ((2, 1, 256, 0, 0, 0, 0, 2),) + SNAP + GEO + SOLVE),
                                   (250000, 1, 20, CHAINS + SNAP + GEO + SOLVE), (4000, 2, 800, GRID)):
        cs, ct = pair(n); ctx.tune("nn_method", method)
        us = {a: [] for a in arms}
        poses, chains = {}, {}
        for r in range(reps + 1):                      # (the first round warms up: indexes, spare buffers)
            for a in arms:
                for k_, v_ in zip(KEYS, a):
                    ctx.tune(k_, v_)
                t0 = time.perf_counter()
                T, st = ctx.icp_point2point(cs, ct, max_corr=1.0, max_iter=iters, eps=0.0)
                dt = time.perf_counter() - t0
                if r: us[a].append(dt / max(st["iters_run"], 1) * 1e6)
                poses[a] = T.view(np.uint32).tobytes(); chains[a] = (ctx.icp_last_chain(), ctx.icp_last_snapshots())
        same = all(p == poses[arms[0]] for p in poses.values())
        for a in arms:
            v = np.array(us[a])
            print(f"n={n} method={method} iterations={iters} icp_move_in_search={a[0]} icp_fused_sums={a[1]} threads={a[2]} solve threads={a[3]} pairs={a[4]} "
                  f"host snapshots={a[5]} ticket levels={a[6]} icp_solve_in_search={a[7]} chain {chains[a][0]} snapshots {chains[a][1]}: "
                  f"median {np.median(v):.2f} us/iteration, spread {v.max() - v.min():.2f} "
                  f"(min {v.min():.2f}, max {v.max():.2f}; {reps} calls); pose bits equal: {same}")
        cs.free(); ct.free()
