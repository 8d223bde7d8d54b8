#!/usr/bin/env python3
"""The extended driver (eigsolve_?hegvdx_ex) against the marks of its issue, in one process: median ms of
  * the device bisection (all N eigenvalues, N = 2048 / 4096 / 8192, and the 1024 lowest at N = 4096) against the device divide &
    conquer on the same tridiagonal (the T of the C3-recipe problem at N = 4096 and of same-recipe problems at the other orders);
  * the phases of the C3 (complex N = 4096, m = 1024) and C2 (real N = 2048, m = 512) solves: eigsolve_?hegvdx, the extended entry
    with itype 1 / 2 / 3 and jobz 'V', and jobz 'N' (phase [3] = the bisection there, [5] = the trmm for itype 3).
Usage: python tools/ex_phases.py [reps]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from bench import gen_pair  # noqa: E402
from eigensolver_gpu_amd import api  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
KEYS = ["potrf", "gst", "trd", "stedc_host", "backtransform", "trsm", "total"]


def med(xs):
    return sorted(xs)[len(xs) // 2]


print("== tridiagonal eigenvalues: bisection (stebz) vs divide & conquer (stedc), host wall ms incl. sync, median of %d" % reps)
for n in (2048, 4096, 8192):
    A, _ = gen_pair(n, True, 1002, dev)
    d, e, _ = api.hetrd(A.clone())
    d, e = d.cpu().numpy(), e.cpu().numpy()
    for sub in ((None, None), (1, 1024)) if n == 4096 else ((None, None),):
        tb, td = [], []
        for r in range(reps + 1):
            if sub[0] is None:
                rc, wb, ms = api.stebz_device(d, e, "A")
            else:
                rc, wb, ms = api.stebz_device(d, e, "I", il=sub[0], iu=sub[1])
            assert rc == 0
            rc, wd, _, ms2 = api.stedc_device(d, e)
            assert rc == 0
            if r:
                tb.append(ms)
                td.append(ms2)
        k = len(wb)
        err = np.abs(wb - wd[:k]).max() / np.abs(wd).max()
        print("N=%5d  eigenvalues %5d   stebz %8.3f   stedc(all, with vectors) %8.3f   max|diff|/||T|| %.1e" %
              (n, k, med(tb), med(td), err), flush=True)


def run(label, fn):
    rows = []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        wall = (time.perf_counter() - t0) * 1e3
        if r:
            ph = api.phase_times()
            ph["wall"] = wall
            rows.append(ph)
    print("%-28s %s" % (label, "  ".join("%s %7.3f" % (k, med([x[k] for x in rows])) for k in KEYS + ["wall"])), flush=True)


for name, cplx, n, m in (("C3", True, 4096, 1024), ("C2", False, 2048, 512)):
    print("== %s: %s N=%d m=%d, phase ms (median of %d)" % (name, "complex" if cplx else "real", n, m, reps))
    A0, B0 = gen_pair(n, cplx, 1002, dev)
    ws = api.Workspace(n, cplx)
    for overlap in (3, 0):
        api.set_option("overlap", overlap)

        def base():
            info, _ = api.hegvdx(A0.clone(), B0.clone(), 1, m, ws, skip_host_copy=True)
            assert info == 0
        run("hegvdx (overlap %d)" % overlap, base)
        for itype in (1, 2, 3):
            def ex(itype=itype, jobz="V"):
                info, me, _, _ = api.hegvdx_ex(A0.clone(), B0.clone(), itype=itype, jobz=jobz, range="I", il=1, iu=m, ws=ws)
                assert info == 0 and me == m
            run("ex itype %d V (overlap %d)" % (itype, overlap), ex)
            run("ex itype %d N (overlap %d)" % (itype, overlap), lambda itype=itype: ex(itype, "N"))
    api.set_option("overlap", 3)
