"""GPU tests of the extended generalized driver (eigsolve_?hegvdx_ex): problem types 2 and 3, eigenvalues only (jobz='N'),
value ranges (range='V'), the device bisection (eigsolve_dstebz_device) and the itype 2 / 3 reduction (eigsolve_?hegst_ex).

Tolerances (fp64): eigenvalues of the bisection as test_stedc_device_vs_lapack; end to end, well-conditioned pencils (B += N*I):
eigenvalues within 1e-12 of LAPACK relative to the largest, residual of the problem's own equation normalised by its operands
<= N*eps, normalisation (Z^H B Z = I for itype 1, 2; Z^H B^-1 Z = I for itype 3) <= 1e-12 (1e-10 at full size).
"""
import numpy as np
import pytest

from test_gpu_parity import _tridiag_cases, env  # noqa: F401  (the shared fixture and matrix families)

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def _gap_midpoints(wr):
    """(vl, vu) at the midpoints of the widest gap in each half of the spectrum (all of it when there is no gap)."""
    n = len(wr)
    g = np.diff(wr)
    if n < 3 or g.max() <= 0:
        return wr.min() - 1.0, wr.max() + 1.0
    h = max(1, (n - 1) // 2)
    i = int(np.argmax(g[:h]))
    j = h + int(np.argmax(g[h:]))
    return 0.5 * (wr[i] + wr[i + 1]), 0.5 * (wr[j] + wr[j + 1])


@pytest.mark.parametrize("case", _tridiag_cases(), ids=lambda c: c[0])
def test_stebz_device_vs_lapack(env, case):  # noqa: F811
    """All eigenvalues, index subsets and value subsets of the device bisection against LAPACK on every matrix family of the
    divide & conquer test: the same eigenvalue bound, ascending output, exact counts, bitwise-repeatable calls."""
    torch, oracle, api = env
    from scipy.linalg import eigh_tridiagonal
    name, d, e = case
    n = len(d)
    wr = eigh_tridiagonal(d, e, eigvals_only=True) if n > 1 else d.copy()
    nrm = max(np.abs(wr).max(), 1e-300)
    bound = 50 * max(n, 8) * EPS / 8
    rc, w, _ = api.stebz_device(d, e, "A")
    assert rc == 0 and len(w) == n
    assert np.all(np.diff(w) >= 0)
    assert np.abs(w - wr).max() / nrm <= bound
    rc2, w2, _ = api.stebz_device(d, e, "A")
    assert rc2 == 0 and np.array_equal(w, w2)
    # index subset (il > 1): the same bits as the full call
    il, iu = (n + 3) // 4, max((n + 3) // 4, (3 * n) // 4)
    rc, wi, _ = api.stebz_device(d, e, "I", il=il, iu=iu)
    assert rc == 0 and np.array_equal(wi, w[il - 1:iu])
    # value subset with vl, vu at gap midpoints: the count is LAPACK's
    vl, vu = _gap_midpoints(wr)
    rc, wv, _ = api.stebz_device(d, e, "V", vl=vl, vu=vu)
    sel = wr[(wr > vl) & (wr <= vu)]
    assert rc == 0 and len(wv) == len(sel)
    if len(sel):
        assert np.abs(wv - sel).max() / nrm <= bound
    # an empty value range
    lo = wr.max() + 1.0 + abs(wr.max())
    rc, we, _ = api.stebz_device(d, e, "V", vl=lo, vu=2 * lo + 1.0)
    assert rc == 0 and len(we) == 0


# ---------------------------------------------------------------------------------------------
# the itype 2 / 3 reduction
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("n", [1, 33, 64, 65, 257, 1000])
def test_hegst_ex_vs_lapack(env, cplx, n):  # noqa: F811
    """hegst_ex(2|3) = LAPACK ?hegst(itype 2|3) (both form U A U^H), lda > n, NaN-poisoned strict lower triangle kept."""
    torch, oracle, api = env
    import scipy.linalg as sl
    import scipy.linalg.lapack as ll
    A = oracle.gen_spd(n, 300 + n, cplx)
    B = oracle.gen_spd(n, 400 + n, cplx, shift=float(n))
    U = np.triu(sl.cholesky(B, lower=False))
    hegst = ll.zhegst if cplx else ll.dsygst
    lda = n + 7
    for itype in (2, 3):
        ref, info = hegst(A, U, itype=itype, lower=0)
        assert info == 0
        Ap = np.full((lda, n), np.nan, dtype=A.dtype)
        Ap[:n] = np.triu(A) + np.tril(np.full((n, n), np.nan), -1)
        Ad = api.to_device(Ap)
        assert api.hegst_ex(itype, Ad, api.to_device(U)) == 0
        out = api.to_host(Ad)
        iu_ = np.triu_indices(n)
        got, want = out[:n][iu_], np.triu(ref)[iu_]
        assert np.abs(got - want).max() <= 200 * n * EPS * np.abs(want).max()
        assert np.all(np.isnan(out[:n][np.tril_indices(n, -1)]))
        assert np.all(np.isnan(out[n:]))
    # itype 1 through the same entry is ?hegst(1)
    ref, info = hegst(A, U, itype=1, lower=0)
    Ad = api.to_device(np.triu(A))
    assert api.hegst_ex(1, Ad, api.to_device(U)) == 0
    got = np.triu(api.to_host(Ad))
    assert np.abs(got - np.triu(ref)).max() <= 200 * n * EPS * np.abs(np.triu(ref)).max()


# ---------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------
def _pencil(oracle, n, cplx, seed):
    A = oracle.gen_spd(n, seed + n, cplx)
    B = oracle.gen_spd(n, seed + 1000 + n, cplx, shift=float(n))
    return A, B


def _residual(itype, A, B, w, Z):
    """||op Z - Z diag(w)|| / (||A|| ||B|| ||Z||) for itype 2 / 3, ||A Z - B Z diag(w)|| / ||A|| for itype 1."""
    if itype == 1:
        return np.linalg.norm(A @ Z - (B @ Z) * w[None, :]) / np.linalg.norm(A)
    R = (A @ (B @ Z) if itype == 2 else B @ (A @ Z)) - Z * w[None, :]
    return np.linalg.norm(R) / (np.linalg.norm(A) * np.linalg.norm(B) * max(np.linalg.norm(Z), 1e-300))


def _normalisation(itype, B, Z):
    G = Z.conj().T @ (np.linalg.solve(B, Z) if itype == 3 else B @ Z)
    return np.linalg.norm(G - np.eye(Z.shape[1]))


def _solve(api, A, B, **kw):
    Ad, Bd = api.to_device(np.triu(A)), api.to_device(np.triu(B))
    info, m, w, Z = api.hegvdx_ex(Ad, Bd, **kw)
    return info, m, w.cpu().numpy().copy(), (np.asfortranarray(api.to_host(Z)) if Z is not None else None), Ad, Bd


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("n", [1, 40, 130, 257, 700])
@pytest.mark.parametrize("itype", [1, 2, 3])
def test_hegvdx_ex_vs_lapack(env, cplx, n, itype):  # noqa: F811
    """Every (jobz, range) against scipy.linalg.eigh(type=itype): counts, eigenvalues, the residual of the problem's own
    equation and LAPACK's normalisation; il > 1 for the index range."""
    torch, oracle, api = env
    import scipy.linalg as sl
    A, B = _pencil(oracle, n, cplx, 5000 * itype)
    wl = sl.eigh(A, B, type=itype, eigvals_only=True)
    nrm = np.abs(wl).max()
    il, iu = (max(1, n // 5), max(1, n // 2)) if n > 1 else (1, 1)
    vl, vu = _gap_midpoints(wl)
    for rng_ in ("A", "I", "V"):
        if rng_ == "A":
            want = wl
        elif rng_ == "I":
            want = wl[il - 1:iu]
        else:
            want = wl[(wl > vl) & (wl <= vu)]
        for jobz in ("N", "V"):
            info, m, w, Z, _, _ = _solve(api, A, B, itype=itype, jobz=jobz, range=rng_, vl=vl, vu=vu, il=il, iu=iu)
            assert info == 0, (rng_, jobz)
            assert m == len(want), (rng_, jobz, m, len(want))
            assert np.all(np.diff(w) >= 0)
            assert np.abs(w - want).max() / nrm <= 1e-12, (rng_, jobz)
            if jobz == "V":
                assert Z.shape == (n, m)
                assert _residual(itype, A, B, w, Z) <= max(n, 4) * EPS, (rng_, jobz)
                assert _normalisation(itype, B, Z) <= 1e-12, (rng_, jobz)
            else:
                assert Z is None


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("overlap", [0, 3])
@pytest.mark.parametrize("n,il,iu", [(300, 1, 300), (700, 100, 274)])
def test_itype1_bit_identical_to_hegvdx(env, cplx, overlap, n, il, iu):  # noqa: F811
    """itype 1, jobz 'V', range 'I' / 'A' runs the launches of eigsolve_?hegvdx: Z and the selected w are the same bits."""
    torch, oracle, api = env
    A, B = _pencil(oracle, n, cplx, 77)
    api.set_option("overlap", overlap)
    try:
        info, ws = api.hegvdx(api.to_device(np.triu(A)), api.to_device(np.triu(B)), il, iu, skip_host_copy=True)
        assert info == 0
        m = iu - il + 1
        Zr = ws.Z[:m].cpu().numpy().copy()
        wr = ws.w.cpu().numpy()[il - 1:iu].copy()
        for rng_ in (("A",) if m == n else ()) + ("I",):
            ws2 = api.Workspace(n, cplx, pinned=False)
            info, me, w, Z = api.hegvdx_ex(api.to_device(np.triu(A)), api.to_device(np.triu(B)), itype=1, jobz="V", range=rng_,
                                           il=il, iu=iu, ws=ws2)
            assert info == 0 and me == m
            assert np.array_equal(w.cpu().numpy(), wr)
            assert np.array_equal(Z.cpu().numpy(), Zr)
    finally:
        api.set_option("overlap", 3)


@pytest.mark.parametrize("cplx", [False, True])
def test_jobz_n_matches_jobz_v_and_null_z(env, cplx):  # noqa: F811
    """Eigenvalues only vs with vectors on one problem (within the bisection bound), Z_d = NULL accepted for jobz 'N'."""
    torch, oracle, api = env
    n = 257
    for itype in (1, 2, 3):
        A, B = _pencil(oracle, n, cplx, 900 + itype)
        info, m, wn, Z, _, _ = _solve(api, A, B, itype=itype, jobz="N", range="A")
        assert info == 0 and m == n and Z is None
        info, m2, wv, _, _, _ = _solve(api, A, B, itype=itype, jobz="V", range="A")
        assert info == 0 and m2 == n
        assert np.abs(wn - wv).max() / np.abs(wv).max() <= 50 * n * EPS


@pytest.mark.parametrize("cplx", [False, True])
def test_itype3_column_chunked_path(env, cplx):  # noqa: F811
    """itype 3 with the eigenvector block capped (zs_cap_mb): the chunked back-transformation gives the unchunked result."""
    torch, oracle, api = env
    n = 700
    A, B = _pencil(oracle, n, cplx, 31)
    for rng_, kw in (("I", dict(il=3, iu=600)), ("V", {})):
        if rng_ == "V":
            import scipy.linalg as sl
            kw = dict(zip(("vl", "vu"), _gap_midpoints(sl.eigh(A, B, type=3, eigvals_only=True))))
        info, m, w, Z, _, _ = _solve(api, A, B, itype=3, jobz="V", range=rng_, **kw)
        assert info == 0 and m > 0
        api.set_option("zs_cap_mb", 1)
        try:
            info2, m2, w2, Z2, _, _ = _solve(api, A, B, itype=3, jobz="V", range=rng_, **kw)
        finally:
            api.set_option("zs_cap_mb", 4096)
        assert info2 == 0 and m2 == m
        assert np.array_equal(w, w2)
        assert np.abs(Z - Z2).max() <= 1e-12 * np.abs(Z).max()
        assert _residual(3, A, B, w2, Z2) <= n * EPS


@pytest.mark.parametrize("cplx", [False, True])
def test_empty_value_range(env, cplx):  # noqa: F811
    torch, oracle, api = env
    n = 130
    A, B = _pencil(oracle, n, cplx, 41)
    for itype in (1, 2, 3):
        for jobz in ("N", "V"):
            info, m, w, Z, _, _ = _solve(api, A, B, itype=itype, jobz=jobz, range="V", vl=-2.0, vu=-1.0)
            assert info == 0 and m == 0 and len(w) == 0


@pytest.mark.parametrize("cplx", [False, True])
def test_rejected_arguments_leave_inputs_unmodified(env, cplx):  # noqa: F811
    """Every rejected argument gives info -1 before any device work; B not positive definite gives info -1."""
    torch, oracle, api = env
    n = 48
    A, B = _pencil(oracle, n, cplx, 51)
    bad = [dict(itype=0), dict(itype=4), dict(jobz="X"), dict(range="Q"), dict(range="V", vl=1.0, vu=1.0),
           dict(range="V", vl=2.0, vu=1.0), dict(range="I", il=0, iu=3), dict(range="I", il=5, iu=4),
           dict(range="I", il=1, iu=n + 1)]
    for kw in bad:
        Ad, Bd = api.to_device(np.triu(A)), api.to_device(np.triu(B))
        A0, B0 = Ad.clone(), Bd.clone()
        info, m, _, _ = api.hegvdx_ex(Ad, Bd, **kw)
        assert info == -1 and m == 0, kw
        assert torch.equal(Ad, A0) and torch.equal(Bd, B0), kw
    ws = api.Workspace(n, cplx)
    ws.lwork -= 1
    Ad, Bd = api.to_device(np.triu(A)), api.to_device(np.triu(B))
    A0, B0 = Ad.clone(), Bd.clone()
    info, m, _, _ = api.hegvdx_ex(Ad, Bd, itype=2, ws=ws)
    assert info == -1 and torch.equal(Ad, A0) and torch.equal(Bd, B0)
    Bbad = B.copy()
    Bbad[10, 10] = -1.0
    for itype in (1, 2, 3):
        info, m, _, _ = api.hegvdx_ex(api.to_device(np.triu(A)), api.to_device(np.triu(Bbad)), itype=itype, jobz="N")
        assert info == -1


# ---------------------------------------------------------------------------------------------
# full size (BASELINE C3 / C2 shapes), well-conditioned pencils
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [("C3", True, 4096, 1024), ("C2", False, 2048, 512)], ids=lambda c: c[0])
def test_full_size_itype23(env, cfg):  # noqa: F811
    torch, oracle, api = env
    name, cplx, n, m = cfg
    A = oracle.gen_spd_fast(n, 1000 + n, cplx)
    B = oracle.gen_spd_fast(n, 2000 + n, cplx, shift=float(n))
    Ah = torch.from_numpy(np.ascontiguousarray(A)).cuda()
    Bh = torch.from_numpy(np.ascontiguousarray(B)).cuda()
    nA, nB = torch.linalg.norm(Ah), torch.linalg.norm(Bh)
    ws = api.Workspace(n, cplx, pinned=False)
    for itype in (2, 3):
        info, me, w, Z = api.hegvdx_ex(api.to_device(np.triu(A)), api.to_device(np.triu(B)), itype=itype, jobz="V", range="I",
                                       il=1, iu=m, ws=ws)
        assert info == 0 and me == m
        Zc = Z[:, :n].T            # n x m on the device (the column-major view transposed)
        wv = w.clone()
        assert bool((wv[1:] >= wv[:-1]).all())
        R = (Ah @ (Bh @ Zc) if itype == 2 else Bh @ (Ah @ Zc)) - Zc * wv.to(Zc.dtype)[None, :]
        res = float(torch.linalg.norm(R) / (nA * nB * torch.linalg.norm(Zc)))
        G = Zc.conj().T @ (torch.linalg.solve(Bh, Zc) if itype == 3 else Bh @ Zc)
        nrmz = float(torch.linalg.norm(G - torch.eye(m, device="cuda", dtype=G.dtype)))
        assert res <= n * EPS, (itype, res)
        assert nrmz <= 1e-10, (itype, nrmz)
        wN = api.hegvdx_ex(api.to_device(np.triu(A)), api.to_device(np.triu(B)), itype=itype, jobz="N", range="I", il=1, iu=m,
                           ws=api.Workspace(n, cplx, pinned=False))
        assert wN[0] == 0 and wN[1] == m
        # (both tridiagonal solvers are accurate to eps ||T||, and ||T|| = ||U A U^H|| reaches ||A|| ||B||, far above the
        #  selected eigenvalues)
        assert float((wN[2] - wv).abs().max() / (nA * nB)) <= 50 * n * EPS


def test_fortran_ex_driver(env):  # noqa: F811
    """zhegvdx_ex_gpu / dsygvdx_ex_gpu from Fortran against host ?hegvd(itype) for every (itype, jobz, range)."""
    import os
    import subprocess
    torch, oracle, api = env
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eigensolver_gpu_amd", "fortran",
                       "test_hegvdx_ex")
    if not os.path.exists(exe):
        pytest.skip("Fortran driver not built (amdflang missing at build time)")
    envv = dict(os.environ, EIGSOLVE_LAPACK_LIB=api.find_host_lapack() or "")
    out = subprocess.run([exe], capture_output=True, text=True, env=envv, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "PASSED" in out.stdout
