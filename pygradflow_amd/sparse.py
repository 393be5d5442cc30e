"""Host-side plan of the sparse (banded) mode.

For a FIXED sparsity pattern of H (n x n) and J (m x n) the plan holds a
bandwidth-reducing symmetric permutation of the full (n + m) KKT pattern (reverse
Cuthill-McKee, scipy.sparse.csgraph) and, for every stored entry of H and J, its slot in
the lower band of the permuted matrix.  This is host logic done once per pattern; all
per-step arithmetic (CSR products, band assembly, banded LDL^T, solves, update) runs in
libpgf_hip.so (csrc/pgf_sparse.hip).  Active variables keep their row / column as an
identity row, so the plan survives any churn of the active-set mask.

Replaces, for sparse problems, the scipy slicing + ``bmat`` assembly of the reference
(``symmetric_step_solver.py:27-39, 49-77``).
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np
import scipy.sparse as sps
from scipy.sparse.csgraph import reverse_cuthill_mckee

from . import _lib

MAX_BANDWIDTH = 64  # widest block of the cyclic reduction (csrc/pgf_band_wide.hip)
MAX_BORDER = 64     # most border nodes without asking (csrc/pgf_border.hip: S in 32 KB of LDS, one workgroup)
MAX_LARGE_BORDER = 1024  # ... with problem.pgf_border_limit (csrc/pgf_border_large.hip: S by the dense LDL^T)
BLOCK_SIZES = (8, 16, 32, 64)


def block_size_for(bw, forced=None):
    """Block size of the banded solve for half-bandwidth ``bw``: ``forced`` if given, else
    8 for bw <= 8 (8 x 8 cyclic reduction), the smallest of 16, 32, 64 that is >= bw up to 64
    (so 16 for bw 9 .. 10), and None beyond (no banded path).  Every one of these carries the
    accuracy guard."""
    if forced:
        return int(forced)
    if bw <= 8:
        return 8
    for B in BLOCK_SIZES[1:]:
        if bw <= B:
            return B
    return None


def _bandwidth(pat, pos):
    coo = pat.tocoo()
    return int(np.max(np.abs(pos[coo.row] - pos[coo.col]))) if coo.nnz else 0


def _rcm_positions(pat):
    """pos[old] = new under reverse Cuthill-McKee of the symmetric pattern."""
    perm = reverse_cuthill_mckee(sps.csr_matrix(pat), symmetric_mode=True)  # perm[new] = old
    pos = np.empty(pat.shape[0], dtype=np.int64)
    pos[perm] = np.arange(pat.shape[0])
    return pos


def border_limit_of(limit):
    """A border limit as BandPlan and select_border take it: None is MAX_BORDER (the small border,
    as ever), otherwise an integer in MAX_BORDER .. MAX_LARGE_BORDER."""
    if limit is None:
        return MAX_BORDER
    if isinstance(limit, (bool, np.bool_)) or not isinstance(limit, (int, np.integer)) \
            or not MAX_BORDER <= limit <= MAX_LARGE_BORDER:
        raise ValueError(f"pgf_border_limit: {limit!r} (an integer in {MAX_BORDER} .. {MAX_LARGE_BORDER})")
    return int(limit)


def select_border(pat, limit=MAX_BORDER):
    """The automatic border of a symmetric KKT pattern (diagonal present): every node whose degree
    exceeds 2 * MAX_BANDWIDTH -- it fits no band of that half-width -- and then, while reverse
    Cuthill-McKee of the remainder still gives a wider band, the remainder's node of highest
    degree (the highest index among equals: where thousands of nodes tie, as in a uniform band,
    the choice is arbitrary, and what RCM makes of the remainder can depend on it).  Returns (sorted border nodes, fits): fits is False
    when ``limit`` nodes (MAX_BORDER unless given) do not bring the remainder's bandwidth down to
    MAX_BANDWIDTH."""
    limit = border_limit_of(limit)
    N = pat.shape[0]
    pat = sps.csr_matrix(pat)
    deg = np.diff(pat.indptr) - 1
    border = [int(i) for i in np.nonzero(deg > 2 * MAX_BANDWIDTH)[0]]
    if len(border) > limit:
        return sorted(border[:limit]), False
    while True:
        keep = np.ones(N, dtype=bool)
        keep[border] = False
        rem = np.nonzero(keep)[0]
        sub = pat[rem, :][:, rem]
        if rem.size == 0 or _bandwidth(sub, _rcm_positions(sub)) <= MAX_BANDWIDTH:
            return sorted(border), True
        if len(border) >= limit or rem.size <= 1:
            return sorted(border), False
        deg = np.diff(sub.indptr)
        border.append(int(rem[np.nonzero(deg == deg.max())[0][-1]]))


class BandPlan:
    """``border``: None (a plain band, as ever), ``"auto"`` (select_border) or a sequence of KKT
    node indices (``i < n``: variable ``i``; ``n + r``: constraint ``r``) that are kept out of the
    band: K = [[B, C], [C', D]] with the band B of the ``Nb`` other nodes (reverse Cuthill-McKee
    runs on those only) and the border nodes, in ascending order -- variables before constraints
    -- at positions ``Nb .. Nb + k - 1``.  The entries that touch a border node get slots in a
    border store directly behind the band array, which the scatter kernels write like any other
    slot: C as ``Nb x kp`` row-major at ``base_C = (Nb + 1) ldb``, then the lower triangle of D as
    ``kp x kp`` at ``base_D = base_C + Nb kp``; ``kp`` is ``k`` rounded up to a multiple of 16.

    ``border_limit`` (``problem.pgf_border_limit``): the most border nodes, None (64) or 64 .. 1024.
    A border of more than 64 nodes is a LARGE border (csrc/pgf_border_large.hip): ``kp`` is ``k``
    rounded up to a multiple of 64, the store is otherwise the same, and the remainder always
    runs the wide route with the factor / solve split -- block size max(16, block_size_for(bw))
    unless 16, 32 or 64 is forced; a forced 8 and ``split`` = False (``problem.pgf_band_split``) are
    errors."""

    def __init__(self, hess, jac, n, m, block=None, border=None, border_limit=None, split=None):
        if block and int(block) not in BLOCK_SIZES:
            raise ValueError(f"band block size {block}: must be one of {BLOCK_SIZES}")
        self.block = int(block) if block else None  # forced block size (problem.pgf_band_block)
        H = sps.csr_matrix(hess, dtype=np.float64)
        J = sps.csr_matrix(jac, dtype=np.float64) if m > 0 else sps.csr_matrix((0, n), dtype=np.float64)
        H.sum_duplicates()
        J.sum_duplicates()
        H.sort_indices()
        J.sort_indices()
        if H.shape != (n, n) or J.shape != (m, n):
            raise ValueError("derivative shapes do not match the problem")
        self.n, self.m = n, m
        N = n + m
        # symmetric pattern of the full KKT matrix (H's pattern symmetrised, diagonal present)
        Hp = sps.csr_matrix((np.ones(H.nnz), H.indices, H.indptr), shape=(n, n))
        Jp = sps.csr_matrix((np.ones(J.nnz), J.indices, J.indptr), shape=(m, n))
        pat = sps.bmat([[Hp + Hp.T + sps.identity(n), Jp.T], [Jp, sps.identity(m)]], format="csr")
        self.border_limit = limit = border_limit_of(border_limit)
        self.border_spec = border_key(border, border_limit)
        self._border_fits = True
        if border is None:
            nodes = np.zeros(0, dtype=np.int64)
        elif isinstance(border, str):
            if border != "auto":
                raise ValueError(f"pgf_border: {border!r} (\"auto\" or a sequence of KKT node indices)")
            found, self._border_fits = select_border(pat, limit)
            nodes = np.asarray(found, dtype=np.int64)
        else:
            nodes = np.unique(np.asarray(list(border), dtype=np.int64))
            if nodes.size != len(list(border)) or nodes.size == 0 or nodes[0] < 0 or nodes[-1] >= N:
                raise ValueError("pgf_border: distinct KKT node indices in [0, n + m) expected")
            if nodes.size > limit:
                raise ValueError(f"pgf_border: {nodes.size} nodes, at most {limit}")
            if nodes.size >= N:
                raise ValueError("pgf_border: the border must leave a band")
        self.border = nodes.astype(np.int32)
        self.k = k = int(nodes.size)
        self.large = k > MAX_BORDER
        self.kp = kp = (k + 63) // 64 * 64 if self.large else (k + 15) // 16 * 16
        if self.large and self.block == 8:
            raise ValueError("pgf_band_block: a border of more than 64 nodes needs block size 16, 32 or 64")
        if self.large and split is not None and not split:
            raise ValueError("pgf_band_split: a border of more than 64 nodes needs the factor / solve split")
        self.Nb = Nb = N - k
        if k == 0:
            pos = _rcm_positions(pat)
            self.bw = _bandwidth(pat, pos)
        else:
            keep = np.ones(N, dtype=bool)
            keep[nodes] = False
            rem = np.nonzero(keep)[0]
            sub = pat[rem, :][:, rem]
            sub_pos = _rcm_positions(sub)
            pos = np.empty(N, dtype=np.int64)
            pos[rem] = sub_pos
            pos[nodes] = Nb + np.arange(k)
            self.bw = _bandwidth(sub, sub_pos)
        self.ldb = (self.bw + 1 + 1) // 2 * 2
        self.pos = pos.astype(np.int32)
        self.base_C = (Nb + 1) * self.ldb
        self.base_D = self.base_C + Nb * kp
        self.store_size = self.base_D + kp * kp if k else (N + 1) * self.ldb
        if k and self.store_size >= 2 ** 31:
            raise ValueError("bordered band: band and border store exceed 2^31 entries")

        def slot(pa, pb):
            """Slot of the entry between positions pa, pb: band, C or the lower triangle of D."""
            a, lo = np.maximum(pa, pb), np.minimum(pa, pb)
            band = a * self.ldb + (a - lo)
            if k == 0:
                return band
            in_c = self.base_C + lo * kp + (a - Nb)
            in_d = self.base_D + (a - Nb) * kp + (lo - Nb)
            return np.where(a < Nb, band, np.where(lo < Nb, in_c, in_d))

        # H entries: lower part in permuted order gets a slot, the mirror is skipped.  An
        # unsymmetric *pattern* (entry (i, j) stored without (j, i)) keeps its only copy.
        hrow = np.repeat(np.arange(n), np.diff(H.indptr))
        hcol = H.indices
        pi, pj = pos[hrow], pos[hcol]
        lower = pi >= pj
        mirror_present = np.asarray(Hp[hcol, hrow]).ravel() > 0
        use = lower | ~mirror_present
        self.Hslot = np.where(use, slot(pi, pj), -1).astype(np.int32)
        self.Hptr = H.indptr.astype(np.int32)
        self.Hrow = hrow.astype(np.int32)
        self.Hcol = hcol.astype(np.int32)
        # J entries: K[n + r][j] or its mirror, whichever is below the diagonal
        jrow = np.repeat(np.arange(m), np.diff(J.indptr))
        jcol = J.indices
        pa, pb = pos[n + jrow], pos[jcol]
        self.Jslot = slot(pa, pb).astype(np.int32)
        self.Jptr = J.indptr.astype(np.int32)
        self.Jcol = jcol.astype(np.int32)
        # column-ordered copy of J's pattern for J' w without atomics
        order = np.lexsort((jrow, jcol))
        self.JTrow = jrow[order].astype(np.int32)
        self.JTmap = order.astype(np.int32)
        self.JTptr = np.concatenate(([0], np.cumsum(np.bincount(jcol, minlength=n)))).astype(np.int32)
        self.nnzH, self.nnzJ = int(H.nnz), int(J.nnz)
        self._Hpat = (H.indptr.copy(), H.indices.copy())
        self._Jpat = (J.indptr.copy(), J.indices.copy())

    @property
    def supported(self) -> bool:
        return self.bw <= MAX_BANDWIDTH and self._border_fits

    @property
    def block_size(self):
        """Block size the solve runs with (block_size_for; at least 16 under a large border)."""
        B = block_size_for(self.bw, self.block)
        return max(16, B) if self.large and B else B

    def values(self, hess, jac):
        """Values of H, J in plan order; raises if the pattern differs from the plan's."""
        H = sps.csr_matrix(hess, dtype=np.float64)
        H.sum_duplicates()
        H.sort_indices()
        if H.nnz != self.nnzH or not (np.array_equal(H.indptr, self._Hpat[0])
                                      and np.array_equal(H.indices, self._Hpat[1])):
            H = self._conform(H, self._Hpat, (self.n, self.n))
        if self.m > 0:
            J = sps.csr_matrix(jac, dtype=np.float64)
            J.sum_duplicates()
            J.sort_indices()
            if J.nnz != self.nnzJ or not (np.array_equal(J.indptr, self._Jpat[0])
                                          and np.array_equal(J.indices, self._Jpat[1])):
                J = self._conform(J, self._Jpat, (self.m, self.n))
            jv = np.ascontiguousarray(J.data, dtype=np.float64)
        else:
            jv = np.zeros(0)
        return np.ascontiguousarray(H.data, dtype=np.float64), jv

    @staticmethod
    def _conform(mat, pat, shape):
        """Re-express ``mat`` on the plan's pattern (entries outside it are an error)."""
        ptr, idx = pat
        base = sps.csr_matrix((np.zeros(len(idx)), idx, ptr), shape=shape)
        full = (base + mat).tocsr()
        full.sort_indices()
        if full.nnz != len(idx):
            raise ValueError("sparsity pattern changed: rebuild the band plan")
        out = sps.csr_matrix((np.zeros(len(idx)), idx, ptr), shape=shape)
        out.data = np.asarray(full.data, dtype=np.float64)
        return out

    def pattern_hash(self, lib=None):
        """The 64-bit hash a handle keeps of this plan's pattern (``pgf_sparse_pattern_hash``, host
        only): the instances of a banded device batch must agree in it."""
        lib = _lib.load() if lib is None else lib
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
        out = C.c_uint64(0)
        rc = lib.pgf_sparse_pattern_hash(
            self.n, self.m, self.bw, ip(self.pos), self.nnzH, ip(self.Hptr), ip(self.Hrow), ip(self.Hcol),
            ip(self.Hslot), self.nnzJ, ip(self.Jptr), ip(self.Jcol), ip(self.Jslot), ip(self.JTptr),
            ip(self.JTrow), ip(self.JTmap), C.byref(out))
        _lib.check(rc, None, "pgf_sparse_pattern_hash")
        return out.value

    def upload(self, lib, handle):
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
        rc = lib.pgf_sparse_set_pattern(
            handle, self.bw, ip(self.pos), self.nnzH, ip(self.Hptr), ip(self.Hrow), ip(self.Hcol),
            ip(self.Hslot), self.nnzJ, ip(self.Jptr), ip(self.Jcol), ip(self.Jslot), ip(self.JTptr),
            ip(self.JTrow), ip(self.JTmap))
        _lib.check(rc, handle, "pgf_sparse_set_pattern")
        if self.large:  # the wide route first: the large border is declared on it
            rc = lib.pgf_sparse_set_block_size(handle, self.block_size)
            _lib.check(rc, handle, f"pgf_sparse_set_block_size (half-bandwidth {self.bw})")
            _lib.check(lib.pgf_sparse_set_border_large(handle, self.k), handle, "pgf_sparse_set_border_large")
            return
        if self.k:
            _lib.check(lib.pgf_sparse_set_border(handle, self.k), handle, "pgf_sparse_set_border")
        rc = lib.pgf_sparse_set_block_size(handle, self.block or 0)
        _lib.check(rc, handle, f"pgf_sparse_set_block_size (half-bandwidth {self.bw})")


def band_split(problem):
    """``problem.pgf_band_split``: the factor / solve split of the wide banded solve
    (``pgf_sparse_set_factor_split``).  None (not set): the library's default stays; otherwise a
    bool (or 0 / 1)."""
    v = getattr(problem, "pgf_band_split", None)
    if v is None:
        return None
    if isinstance(v, (bool, np.bool_)) or (isinstance(v, (int, np.integer)) and v in (0, 1)):
        return bool(v)
    raise ValueError(f"pgf_band_split must be a bool, not {v!r}")


def _band_split_default():
    """The library's default (``PGF_BW_SPLIT=0`` switches it off; pgf_api_band_setup.hip reads it alike)."""
    v = os.environ.get("PGF_BW_SPLIT")
    if v is None:
        return True
    try:
        return int(v.strip() or 0) != 0
    except ValueError:
        return False  # (atoi of a non-number is 0)


def effective_band_split(problem):
    """The split the problem's handle will run with: ``problem.pgf_band_split`` or, if not set, the
    library's default.  What BandPlan(split=...) needs to refuse a large border in time."""
    want = band_split(problem)
    return _band_split_default() if want is None else want


def apply_band_split(lib, handle, problem):
    """Set the handle's split to what the problem asks for, or back to the default: pooled handles
    keep what their last user set.  A handle that still carries a LARGE border cannot run without
    the split: the border is removed first and True returned -- the caller's plan for the handle is
    stale and is built again (which raises, if it is a large border that the split was switched off
    under)."""
    want = band_split(problem)
    on = _band_split_default() if want is None else want
    dropped = False
    if not on:
        k = C.c_int(0)
        _lib.check(lib.pgf_debug_border_stats(handle, C.byref(k), None, None), handle, "pgf_debug_border_stats")
        if k.value > MAX_BORDER:
            _lib.check(lib.pgf_sparse_set_border(handle, 0), handle, "pgf_sparse_set_border")
            dropped = True
    _lib.check(lib.pgf_sparse_set_factor_split(handle, int(on)), handle, "pgf_sparse_set_factor_split")
    return dropped


def border_key(border, limit=None):
    """Hashable form of a ``problem.pgf_border`` setting (None, "auto" or node indices) and, if one is
    set, of ``problem.pgf_border_limit``: a handle's plan is rebuilt when it differs."""
    key = border if border is None or isinstance(border, str) else tuple(int(i) for i in border)
    return key if limit is None else ("limit", int(limit), key)


def wants_band(problem, hess, n, m, dense_limit=20000):
    """Sparse derivatives take the banded path when the problem is too large for the dense
    one, or when the problem asks for it (``pgf_force_band``; tests use that).  A problem may
    also force the block size of the banded solve (``pgf_band_block``: 8, 16, 32 or 64, at
    least the half-bandwidth)."""
    if not sps.issparse(hess):
        return False
    return bool(getattr(problem, "pgf_force_band", False)) or (n + m > dense_limit)
