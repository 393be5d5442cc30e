"""The lazy trailing-update plan of the dense LDL^T, walked on the host (CPU).

``pgf_debug_update_plan`` returns the jobs ``plan_updates`` gives every launch and, tile number
by tile number, what ``upd_tile`` -- the function the device workers run -- makes of them.

Blocks are 256 wide; a pre-eliminated block of depth ``vdepth`` counts as ``nv = ceil(vdepth /
256)`` virtual blocks in front: unified block ``p < nv`` is virtual, real block ``k`` is ``p = nv
+ k``.  Column block ``J`` takes the blocks ``p < nv + J``.  The jobs of stage ``s`` run beside
the diagonal chain D(s + 1), stage -1 beside D(0).  Two pieces are not the plan's: the virtual
blocks' update of the first diagonal block (``k_virtual_diag``) and block ``J - 1``'s update of
diagonal block ``J`` (``k_update_diag`` / ``k_trsm_ud``).
"""

import ctypes as C

import numpy as np
import pytest

OB = 256
TM = 64  # UPD_TM: rows of a tile (x 128 columns)
MAXJOBS = 96  # UPD_MAXJOBS
JOB_INTS = 10  # PGF_UPDATE_PLAN_JOB_INTS
STAGE, COL0, NTC, ROWSTART, KC0V, KBV, KC0, KB, T0, T1 = range(JOB_INTS)
SEARCHED = range(400, 2801, 40)  # the budgets the production search tries (besides "no limit")

PRODUCTION = (-1, 0)
CHOICES = (PRODUCTION, (0, 2), (40, 1), (420, 2), (420, 4))
CHOICE_IDS = ["production", "eager_cap2", "b40_cap1", "b420_cap2", "b420_cap4"]


def _plan(N, nrows, vdepth, budget, cap, tiles=True):
    """(jobs [n, 10], tiles [n, 4] or None, jobs per stage [nblk], budget of the plan)"""
    from pygradflow_amd import _lib

    lib = _lib.load()
    ip = C.POINTER(C.c_int)
    nblk = (N + OB - 1) // OB
    nj, nt, bo = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    per_stage = np.full(nblk, -1, dtype=np.int32)
    rc = lib.pgf_debug_update_plan(N, nrows, vdepth, budget, cap, None, 0, C.byref(nj), None, 0, None,
                                   per_stage.ctypes.data_as(ip), C.byref(bo))
    assert rc == 0
    jobs = np.zeros((max(nj.value, 1), JOB_INTS), dtype=np.int32)
    # room for a few tiles more than the tables announce: a walk that ran past a table's end shows
    ntab = 0
    tl = None
    if tiles:
        rc = lib.pgf_debug_update_plan(N, nrows, vdepth, budget, cap, jobs.ctypes.data_as(ip), len(jobs),
                                       None, None, 0, None, None, None)
        assert rc == 0
        ntab = sum(int(jobs[:nj.value][jobs[:nj.value, STAGE] == s, T1].max(initial=0))
                   for s in range(-1, nblk - 1))
        tl = np.full((ntab + 16, 4), -7, dtype=np.int32)
    nj2 = C.c_int(-1)
    rc = lib.pgf_debug_update_plan(N, nrows, vdepth, budget, cap, jobs.ctypes.data_as(ip), len(jobs),
                                   C.byref(nj2), tl.ctypes.data_as(ip) if tiles else None,
                                   len(tl) if tiles else 0, C.byref(nt), None, None)
    assert rc == 0 and nj2.value == nj.value
    jobs = jobs[:nj.value]
    if tiles:
        # the walk stops where upd_tile itself reports the end: one tile more and the first number
        # past a table's end did not decode to "past the end"
        assert nt.value == ntab
        tl = tl[:ntab]
    assert per_stage.sum() == len(jobs)
    return jobs, tl, per_stage, bo.value


def _blocks(job, nv, vdepth):
    """unified blocks of a job's K-range; checks that it is a run of whole blocks"""
    kc0v, kbv, kc0, kb = (int(job[f]) for f in (KC0V, KBV, KC0, KB))
    assert kc0 % OB == 0 and kb % OB == 0 and kc0v % OB == 0 and kb >= 0 and kbv >= 0
    assert kbv % OB == 0 or kc0v + kbv == vdepth
    assert kc0v + kbv <= vdepth
    assert kb + kbv > 0
    ps = []
    if kbv > 0:
        ps += list(range(kc0v // OB, (kc0v + kbv + OB - 1) // OB))
    if kb > 0:
        ps += [nv + k for k in range(kc0 // OB, (kc0 + kb) // OB)]
    # virtual segment first, then the real one: contiguous only if both meet at nv
    assert ps == list(range(ps[0], ps[0] + len(ps)))
    return ps


def _check_jobs_common(jobs, per_stage, N, vdepth):
    nblk = (N + OB - 1) // OB
    assert len(per_stage) == nblk
    assert per_stage.max(initial=0) <= MAXJOBS
    if vdepth == 0:
        assert per_stage[0] == 0  # no stage -1 without virtual blocks
    for s in range(-1, nblk - 1):
        js = jobs[jobs[:, STAGE] == s]
        assert len(js) == per_stage[s + 1]
        if len(js) == 0:
            continue
        depth = js[:, KB] + js[:, KBV]
        assert np.all(depth[:-1] >= depth[1:])  # deepest first
        # tile numbers: contiguous from 0
        assert np.all(js[:, T0] == np.concatenate(([0], js[:-1, T1])))
        assert np.all(js[:, T1] > js[:, T0])
        # (c) no panel that does not exist yet
        if s >= 0:
            assert np.all(js[:, KC0] + js[:, KB] <= OB * (s + 1))
        else:
            assert np.all(js[:, KB] == 0)
    assert set(np.unique(jobs[:, STAGE])) <= set(range(-1, nblk - 1))


@pytest.mark.parametrize("choice", CHOICES, ids=CHOICE_IDS)
@pytest.mark.parametrize("vdepth", (0, 32, 256, 288, 768))
@pytest.mark.parametrize("extra_row", (0, 1), ids=["nrows=N", "nrows=N+1"])
@pytest.mark.parametrize("N", (1, 200, 256, 257, 384, 512, 513, 769, 1024, 1100, 1537))
def test_plan_covers_every_block_once_in_time_and_tiles_partition_jobs(N, extra_row, vdepth, choice):
    nrows = N + extra_row
    budget, cap = choice
    jobs, tiles, per_stage, _ = _plan(N, nrows, vdepth, budget, cap)
    _check_jobs_common(jobs, per_stage, N, vdepth)
    nblk, nv, ntcol = (N + OB - 1) // OB, (vdepth + OB - 1) // OB, (N + 127) // 128
    P = nv + nblk
    cnt = np.zeros((nrows, ntcol, P), dtype=np.int16)
    stage_of = np.full((nrows, ntcol, P), -9, dtype=np.int16)  # (the one stage, where cnt == 1)
    expected_tiles = {}
    for s in range(-1, nblk - 1):
        in_stage = np.zeros((nrows, ntcol), dtype=np.int16)
        for q, job in enumerate(jobs[jobs[:, STAGE] == s]):
            ps = _blocks(job, nv, vdepth)
            col0, rowstart = int(job[COL0]), int(job[ROWSTART])
            assert col0 % 128 == 0 and job[NTC] >= 1
            want = []
            for c in range(int(job[NTC])):
                j0 = col0 + 128 * c
                if j0 >= N:
                    continue
                r0 = max(rowstart, j0)
                # (a) the chain D(s + 1) owns its diagonal block during this launch
                if j0 // OB == s + 1:
                    assert r0 >= min(OB * (s + 2), N)
                cnt[r0:nrows, j0 // 128, ps] += 1
                stage_of[r0:nrows, j0 // 128, ps] = s
                in_stage[r0:nrows, j0 // 128] += 1
                want += [(i0, j0) for i0 in range(r0, nrows, TM)]
            assert len(want) == job[T1] - job[T0]
            expected_tiles[(s, q)] = sorted(want)
        assert in_stage.max(initial=0) <= 1  # no two jobs of a launch on one tile

    i = np.arange(nrows)[:, None, None]
    j0 = 128 * np.arange(ntcol)[None, :, None]
    J = j0 // OB
    p = np.arange(P)[None, None, :]
    diag = i < np.minimum(OB * (J + 1), N)  # rows of column block J's diagonal block
    expect = (j0 <= i) & (p < nv + J)
    expect &= ~((J == 0) & (p < nv) & diag)  # k_virtual_diag
    expect &= ~((J >= 1) & (p == nv + J - 1) & diag)  # k_update_diag / k_trsm_ud
    assert np.array_equal(cnt, expect.astype(np.int16))
    # deadlines: (b) everything column block J gets from the plan is there before T(J), i.e. comes
    # from stages <= J - 1; (a) its diagonal block's part before D(J): stages <= J - 2
    Jb, db = np.broadcast_to(J, expect.shape), np.broadcast_to(diag, expect.shape)
    assert np.all(stage_of[expect] <= (Jb - 1)[expect])
    assert np.all(stage_of[expect & db] <= (Jb - 2)[expect & db])

    # the tiles, as the device numbers them
    assert np.all(tiles[:, 2] < nrows) and np.all(tiles[:, 3] < N) and np.all(tiles[:, 2] >= tiles[:, 3])
    got = {}
    for s, q, i0, jj in tiles.tolist():
        got.setdefault((s, q), []).append((i0, jj))
    assert {k: sorted(v) for k, v in got.items()} == expected_tiles


@pytest.mark.parametrize("choice", (PRODUCTION, (0, 2), (40, 1)), ids=["production", "eager_cap2", "b40_cap1"])
@pytest.mark.parametrize("vdepth", (0, 1024))
@pytest.mark.parametrize("N", (30000, 60000))
def test_job_tables_of_large_factorisations_fit_and_cover(N, vdepth, choice):
    """Where a job table would overflow (no GPU test factorises such a size): the jobs alone,
    per column block split into the rows of its diagonal block and the rows below."""
    nrows = N + 1
    jobs, _, per_stage, _ = _plan(N, nrows, vdepth, choice[0], choice[1], tiles=False)
    _check_jobs_common(jobs, per_stage, N, vdepth)
    nblk, nv = (N + OB - 1) // OB, (vdepth + OB - 1) // OB
    P = nv + nblk
    cnt_diag = np.zeros((nblk, P), dtype=np.int32)
    cnt_below = np.zeros((nblk, P), dtype=np.int32)
    late = 0
    for job in jobs:
        ps = _blocks(job, nv, vdepth)
        p0, p1 = ps[0], ps[-1] + 1
        s, col0, rowstart, ntc = (int(job[f]) for f in (STAGE, COL0, ROWSTART, NTC))
        assert col0 % OB == 0 and ntc % 2 == 0
        for Jc in range(col0 // OB, min(col0 // OB + ntc // 2, nblk)):
            end = min(OB * (Jc + 1), N)
            if rowstart <= OB * Jc:
                cnt_diag[Jc, p0:p1] += 1
                late += s > Jc - 2  # (a): before D(Jc), and not beside it
            else:
                assert rowstart == end  # below the diagonal block, nothing else
            cnt_below[Jc, p0:p1] += 1
            late += s > Jc - 1  # (b): before T(Jc)
    assert late == 0
    Jc = np.arange(nblk)[:, None]
    p = np.arange(P)[None, :]
    want = p < nv + Jc
    assert np.array_equal(cnt_below, want.astype(np.int32))  # (row N lies below every block)
    want_diag = want & ~((Jc == 0) & (p < nv)) & ~((Jc >= 1) & (p == nv + Jc - 1))
    assert np.array_equal(cnt_diag, want_diag.astype(np.int32))


@pytest.mark.parametrize("vdepth", (0, 288))
@pytest.mark.parametrize("N", (513, 1100, 4096))
def test_production_choice_is_a_searched_budget_and_repeats(N, vdepth):
    nrows = N + 1
    jobs, _, per_stage, budget = _plan(N, nrows, vdepth, -1, 0, tiles=False)
    assert budget == 0 or budget in SEARCHED
    again = _plan(N, nrows, vdepth, -1, 0, tiles=False)
    assert np.array_equal(jobs, again[0]) and np.array_equal(per_stage, again[2]) and budget == again[3]
    # and it is the plan of that budget with the cap production uses
    same = _plan(N, nrows, vdepth, budget, 4 if vdepth else 2, tiles=False)
    assert np.array_equal(jobs, same[0]) and same[3] == budget
