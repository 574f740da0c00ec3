"""Row independence of the per-row kernels: one metamorphic harness for test_rows_cpu.py (host build) and
test_gpu_rows.py (device).

``clean`` is a finite batch of M rows, ``poisoned`` the same batch with a set P of rows overwritten by a non-finite
value; both go through the same entry point at the same M, so they take the same launch path, tiling and split.

  a. every output row outside P has the same bytes in both runs (or, for the one mechanism whose summation order depends
     on the inputs by design — the screened closure's exact-row list — agrees at that mechanism's own tolerance);
  b. every output of a row in P that depends on the poisoned input is non-finite (NaN or inf, not pinned).

The reference for a poisoned batch is the oracle ROW BY ROW: its batched formulation (a dense M × M posterior covariance
whose zero cotangents meet NaN entries) spreads a NaN over the gradients of the whole batch, which is an artefact of the
formulation and not a behaviour to reproduce.  ``gpis_rows`` builds per-row GPIS data that way for the host entry
points that take it as an input.
"""
import numpy as np

POISONS = {"nan": np.nan, "posinf": np.inf, "neginf": -np.inf}
OVERFLOW = 1e200  # finite, but a squared distance to it overflows: GPIS queries only


def query_sets(M):
    """Poison sets of a query kernel (32 queries per mean workgroup, 128 per std / screen tile): the first row, the
    last one (the row the std and screen kernels' pad rows replicate), and the rows around the tile edges."""
    sets = [(0,), (M - 1,), tuple(sorted({r for r in (31, 32, 127, 128, M - 2) if 0 <= r < M}))]
    out = []
    for s in sets:
        if s and s not in out:
            out.append(s)
    return out


def candidate_sets(E):
    """Poison sets of a candidate kernel: candidate 0 (which closure_combine_kernel's invalid lanes alias), the last
    one, and a pair across a 16-lane boundary."""
    return [(0,), (E - 1,), (15, 16)]


def poison(a, rows, value, at=0):
    """A copy of ``a`` [M, ...] with flat element ``at`` of every row in ``rows`` set to ``value``."""
    b = np.array(a, copy=True)
    b.reshape(b.shape[0], -1)[list(rows), at] = value
    return b


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _rows(a, M):
    a = np.asarray(a)
    assert a.shape[0] == M, (a.shape, M)
    return a.reshape(M, -1)


def clean_mask(M, P):
    keep = np.ones(M, bool)
    keep[list(P)] = False
    return keep


def assert_clean_rows_keep_bits(clean, poisoned, P, M, tag=""):
    """(a): byte for byte, every output, every row outside P."""
    keep = clean_mask(M, P)
    for k in clean:
        a, b = _rows(clean[k], M)[keep], _rows(poisoned[k], M)[keep]
        if not same_bits(a, b):
            bad = np.flatnonzero([not same_bits(x, y) for x, y in zip(a, b)])
            rows = np.flatnonzero(keep)[bad]
            raise AssertionError(f"{tag}: {k} changed in {len(rows)} clean rows (first {rows[:8].tolist()}) "
                                 f"with rows {list(P)} poisoned")


def assert_clean_rows_close(clean, poisoned, P, M, tol, tag=""):
    """(a) at a tolerance: equal finite masks, equal non-finite entries, finite entries within ``tol`` of the largest;
    integer outputs exactly equal."""
    keep = clean_mask(M, P)
    for k in clean:
        a, b = _rows(clean[k], M)[keep], _rows(poisoned[k], M)[keep]
        if not np.issubdtype(a.dtype, np.floating):
            assert np.array_equal(a, b), (tag, k)
            continue
        fa = np.isfinite(a)
        assert np.array_equal(fa, np.isfinite(b)), (tag, k, "finite masks differ")
        assert np.array_equal(a[~fa], b[~fa], equal_nan=True), (tag, k)
        if fa.any():
            err = float(np.abs(a[fa] - b[fa]).max() / max(np.abs(a[fa]).max(), 1e-300))
            if err > 0.0:
                print(f"{tag}: {k} clean rows differ by {err:.3g}")
            assert err <= tol, (tag, k, err)


def assert_poisoned_rows_nonfinite(poisoned, P, M, names=None, tag=""):
    """(b): the named outputs (default: every floating-point one) are non-finite in every element of the rows in P.
    ``names`` may map an output to a boolean mask [len(P), width] of the elements that depend on the poisoned input."""
    names = {k: None for k in poisoned} if names is None else names
    if not isinstance(names, dict):
        names = {k: None for k in names}
    for k, mask in names.items():
        a = _rows(poisoned[k], M)[list(P)]
        if not np.issubdtype(a.dtype, np.floating):
            continue
        fin = np.isfinite(a)
        if mask is not None:
            fin = fin & np.asarray(mask, bool).reshape(fin.shape)
        assert not fin.any(), f"{tag}: {k} is finite in poisoned rows {[P[i] for i in np.flatnonzero(fin.any(1))]}"


def oracle_masks(rows):
    """``names`` of assert_poisoned_rows_nonfinite from the oracle evaluated on each poisoned row ALONE (a list of
    dicts of [1, ...] arrays, in the order of P): an element is required to be non-finite where the oracle's is."""
    return {k: np.stack([~np.isfinite(np.asarray(r[k], np.float64)).reshape(-1) for r in rows]) for k in rows[0]}


def check(clean, poisoned, P, M, dependent=None, tol=None, tag=""):
    if tol is None:
        assert_clean_rows_keep_bits(clean, poisoned, P, M, tag)
    else:
        assert_clean_rows_close(clean, poisoned, P, M, tol, tag)
    assert_poisoned_rows_nonfinite(poisoned, P, M, dependent, tag)


def gpis_rows(X_clean, gp_clean, X, row_oracle):
    """Per-row GPIS data at X from the data ``gp_clean`` at X_clean: a row whose query has the clean run's bits keeps
    the clean data, a non-finite query's data is NaN (what the oracle gives for such a row evaluated alone,
    test_rows_cpu.test_oracle_poisoned_row_alone_is_nan), any other row is evaluated alone by ``row_oracle(x [1, 3])``."""
    X_clean, X = np.asarray(X_clean).reshape(-1, 3), np.asarray(X).reshape(-1, 3)
    out = {k: np.array(v, copy=True) for k, v in gp_clean.items()}
    for r in range(len(X)):
        if same_bits(X[r], X_clean[r]):
            continue
        one = None if not np.isfinite(X[r]).all() else row_oracle(X[r:r + 1])
        for k, v in out.items():
            if r < len(v):
                v[r] = np.nan if one is None else one[k][0]
    return out


def chain_dependence(desc):
    """[n_tips, n_dofs] bool: tip k's position depends on joint j (the joints on the path from tip k's body up to the
    root, body 0, whose pose is the identity), read from a cdx_chain descriptor."""
    dep = np.zeros((desc.n_tips, desc.n_dofs), bool)
    for k in range(desc.n_tips):
        b = desc.tip_body[k]
        while b > 0:
            if desc.bodies[b].dof >= 0:
                dep[k, desc.bodies[b].dof] = True
            b = desc.bodies[b].parent
    return dep
