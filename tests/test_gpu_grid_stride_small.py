"""GPU parity of every kernel's second and later grid-stride passes, at small sizes.

Every combine and copy kernel is a one-wave block that walks tiles with `for (t = map(blockIdx.x, gridDim.x);
t < ntiles; t += gridDim.x)`; launch() (reduce_kernels.hpp) clamps the grid at kMaxGrid = 2^24 blocks, so with
1 KiB tiles a second pass starts at 16 GiB per operand.  With DCCL_MAX_GRID_TEST=G (tile_maps.hpp max_grid, read
once per process) every launch is clamped at G blocks instead, and operands of about 312 KiB = 3 * 104 tiles take
three passes at G = 104 and about 39 at G = 8: the `full` test of reduce_windows_kernel, the `v <= nvec` edge-lane
loads and lane 63's extra vector on a later pass, the owner of reduce_vec_kernel's partial tile (bid == nfull %
grid), in-place destinations whose neighbouring tile another wave wrote a pass earlier, rows_locate under a
stride.  tests/test_tile_maps.py proves the maps cover every tile once under a clamped grid; this file runs what
the kernels do with the mapped index.

One fresh child process per (family, G, shift), with both knobs in its environment.  The child first asserts that
dccl_max_grid_test() is G and dccl_caps_test_shift() is shift, runs every case of the family's plan, counts them
and prints the count; the parent asserts the count against the family's own product.  Every case: operands of raw
bit patterns (rand_inputs), an op that is random per data set, the result bit for bit (any NaN equals any NaN,
fp_equal) against the oracle in the kernel's documented order, every guard byte before and after the destination
still zero, the sources unchanged.

The shapes are the same bytes for every G (G0 = 104, T = a tile of 64 vectors, V = 16 / sizeof(T)); `nvec` is the
vector body the kernel sees, whatever head scalars the destination's offset adds in front of it.  The element-wise
premul kernels walk blocks of 256 elements, not tiles: for the 8-byte dtypes that is 156 blocks, two uneven passes
at G = 104 and about 20 at G = 8."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import test_gpu_forms_small as forms
from tests.test_gpu_forms_small import DTS, ROUTED_CHAIN, ROUTED_SRC, ROW_CLASSES, WINDOWS_OWN, WINDOWS_SRC, esz_of
from tests.test_gpu_parity import dev_bytes, expected, rand_inputs
from tests.test_oracle import fp_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G0 = 104
# (G, shift): 8 is the smallest legal grid (every run map is the identity, about 39 passes); 104 = 64 + 32 + 8 has
# one full run-of-8 group and a partial one, three full run-of-4 groups and a partial one, six full run-of-2 groups
# and a partial one; with shift 8 312 KiB selects the 78 MiB mid-size forms, with shift 10 the 1 GiB row (tuned
# windows forms, loads-first phased with RUN 4, kMultiStraddle k = 8 RUN 4)
SETTINGS = [(8, 0), (104, 0), (104, 8), (104, 10)]
# (nvec, tail): tail "V-1" is V - 1 elements
SHAPES = [(64 * 3 * G0, 0),                       # three full passes
          (64 * 3 * G0 + 1, 0),                   # one live lane on a fourth pass; nfull % G == 0
          (64 * (2 * G0 + G0 // 2) + 63, "V-1"),  # half the blocks take a third pass; one dead lane
          (64 * (3 * G0 - 1) + 33, 1),            # nfull % G == G - 1
          (64 * (2 * G0 + 5) + 7, "V-1")]         # under RUN 4 the extra pass falls to blocks 0, 8, 16, 24 and 1
ALL_DTS = list(range(10))
KS = {"multi": list(range(2, 9)), "chain": list(range(1, 9))}
CLASS_OWN = ["in_place", "own_in_phase"]
COPY_PAIRS = [1, 3, 8]
COPY_OFFS = [(0, 0), (3, 3), (5, 5), (1, 2), (4, 0), (0, 12), (13, 6), (15, 1), (8, 9), (7, 3)]  # test_copy_multi's
COPY_BYTES = 16 * 64 * 3 * G0 + 7
ROWS_BATCHES = [(1, 4), (1, 5), (1, 6), (5, 0), (5, 1), (5, 2), (32, 0), (32, 1)]  # (segments, rows_case seed)
FAMILIES = ["pair", "classes", "windows", "routed", "premul", "copies"]


def _roffs_unaligned(esz):
    return [1] + ([33 + esz // 2] if (33 + esz // 2) % esz else [])


# pair placements by destination offset: (name, send offset); "in_place" is send == recv
def pair_placements(esz):
    at0 = [("aligned", 0), ("in_place", None), ("straddle", 16), ("elem_phase", esz), ("elem_phase_off_line", esz + 16)]
    at_esz = [("in_phase", esz), ("in_place", None), ("straddle", esz + 16), ("elem_phase", 0), ("elem_phase", 2 * esz)]
    out = []
    if esz > 1:
        at0 += [("byte_phase", 1), ("byte_phase_off_line", 19)]
        at_esz += [("byte_phase", esz + 1)]
    out += [(0, p) for p in at0] + [(esz, p) for p in at_esz]
    if esz > 1:
        for roff in _roffs_unaligned(esz):
            out += [(roff, p) for p in (("unaligned", 0), ("unaligned", 5), ("unaligned", roff), ("in_place", None))]
    return out


def scale_placements(esz):
    p = [("in_place", 0, None), ("in_place", esz, None), ("same_phase", esz, esz + 16), ("other_phase", 0, esz)]
    return p + ([("unaligned", 0, 1)] if esz > 1 else [])


def premul_chain_placements(esz):
    p = ["in_phase", "in_phase_head_in_place", "mixed_phase"]
    return p + (["unaligned"] if esz > 1 else [])


def _n(pred):
    return sum(1 for dt in ALL_DTS if pred(esz_of(dt)))


_N1, _N2, _N48 = _n(lambda e: e == 1), _n(lambda e: e == 2), _n(lambda e: e >= 4)  # 2, 2 and 6 dtypes
_COMBOS = {form: len(ks) * len(DTS) for form, ks in KS.items()}  # every k with every dtype wider than a byte
# the six 4- and 8-byte dtypes have two misaligned destination offsets, the two 16-bit ones one
_ROFFS = (6 * 2 + 2 * 1) / 8
EXPECTED_CASES = {
    # per shape: 10 placements for a 1-byte dtype, 7 + 6 + 4 for a 16-bit one, 7 + 6 + 8 for the others
    "pair": len(SHAPES) * (_N1 * 10 + _N2 * 17 + _N48 * 21),
    # destination 128-B aligned and one element in (head scalars), three classes; the chain in place and apart
    "classes": 2 * len(ROW_CLASSES) * (_COMBOS["multi"] + _COMBOS["chain"] * len(CLASS_OWN)),
    "windows": int(_ROFFS * len(WINDOWS_SRC) * (_COMBOS["multi"] + _COMBOS["chain"] * len(WINDOWS_OWN))),
    "routed": 2 * (_COMBOS["multi"] * len(ROUTED_SRC) + _COMBOS["chain"] * len(ROUTED_CHAIN)),
    # scale: placements x 2 scalars x 2 residences per shape and dtype; chain: k = 1..8 with every dtype
    "premul": len(SHAPES) * 4 * (_N1 * 4 + (_N2 + _N48) * 5) + 8 * (_N1 * 3 + (_N2 + _N48) * 4),
    "copies": len(COPY_PAIRS) * len(COPY_OFFS) + len(ROWS_BATCHES),
    "collective": 2,
}


def count_for(shape, dt, doff):
    """Elements of a case: the shape's vector body and tail, and in front of them the head scalars that bring an
    element-aligned destination at byte offset doff (of a 256-B aligned allocation) to its 128-B line."""
    nvec, tail = shape
    esz = esz_of(dt)
    v = 16 // esz
    head = ((-doff) % 128) // esz if doff % esz == 0 else 0
    return head + nvec * v + (v - 1 if tail == "V-1" else tail)


def tiles_of(count, dt, doff):
    """1 KiB tiles of the launch, as the launchers compute them from count, dtype and the destination's offset."""
    esz = esz_of(dt)
    v = 16 // esz
    head = min(((-doff) % 128) // esz, count) if doff % esz == 0 else 0
    return -(-((count - head) // v) // 64)


def combos(form):
    """(slot, k, dt, shape): every k with every dtype wider than a byte, the shape cycling so that every dtype
    meets every shape too."""
    for ki, k in enumerate(KS[form]):
        for d, dt in enumerate(DTS):
            yield ki * len(DTS) + d, k, dt, SHAPES[(ki + d) % len(SHAPES)]


def plan(family):
    """The cases of a family, without data."""
    cases = []
    if family in ("classes", "windows", "routed"):
        for form in ("multi", "chain"):
            for slot, k, dt, shape in combos(form):
                esz = esz_of(dt)
                if family == "classes":
                    roffs = [0, esz]
                    placements = [(s, o) for s in ROW_CLASSES for o in (CLASS_OWN if form == "chain" else ["none"])]
                elif family == "routed":
                    roffs = [0, esz]
                    placements = [(s, "none") for s in ROUTED_SRC] if form == "multi" else ROUTED_CHAIN
                else:
                    roffs = _roffs_unaligned(esz)
                    placements = [(s, o) for s in WINDOWS_SRC for o in (WINDOWS_OWN if form == "chain" else ["none"])]
                for roff in roffs:
                    for src, own in placements:
                        cases.append(dict(form=form, k=k, dt=dt, shape=shape, count=count_for(shape, dt, roff),
                                          roff=roff, src=src, own=own, slot=(slot, roff)))
    elif family == "pair":
        for dt in ALL_DTS:
            for shape in SHAPES:
                for roff, (name, soff) in pair_placements(esz_of(dt)):
                    cases.append(dict(form="pair", dt=dt, shape=shape, count=count_for(shape, dt, roff), roff=roff,
                                      src=name, soff=soff))
    elif family == "premul":
        for dt in ALL_DTS:
            for shape in SHAPES:
                for name, soff, doff in scale_placements(esz_of(dt)):
                    roff = soff if doff is None else doff
                    for si in range(2):
                        for residence in range(2):
                            cases.append(dict(form="scale", dt=dt, shape=shape, count=count_for(shape, dt, roff),
                                              roff=roff, src=name, soff=soff, in_place=doff is None, scalar=si,
                                              residence=residence))
        for ki, k in enumerate(KS["chain"]):
            for d, dt in enumerate(ALL_DTS):
                esz = esz_of(dt)
                shape = SHAPES[(ki + d) % len(SHAPES)]
                for name in premul_chain_placements(esz):
                    # byte offsets of the sends, then of own and of the destination
                    if name == "in_phase":
                        offs, roff = [0] * (k + 1), 0
                    elif name == "in_phase_head_in_place":
                        offs, roff = [esz + 16 * (j % 3) for j in range(k)] + [esz], esz
                    elif name == "mixed_phase":  # element-aligned, the 16-B phases differ
                        offs, roff = [esz * (j % 2) + 16 * j for j in range(k)] + [0], esz
                    else:
                        offs, roff = [j % 2 for j in range(k)] + [esz + 1], 1
                    cases.append(dict(form="premul_chain", k=k, dt=dt, shape=shape, count=count_for(shape, dt, roff),
                                      roff=roff, src=name, offs=offs, in_place=name == "in_phase_head_in_place",
                                      scalar=ki % 2, residence=(ki // 2) % 2))
    elif family == "copies":
        for npairs in COPY_PAIRS:
            for soff, doff in COPY_OFFS:
                cases.append(dict(form="copy_multi", npairs=npairs, soff=soff, doff=doff, nbytes=COPY_BYTES,
                                  tiles=-(-(COPY_BYTES // 16 + 1) // 64)))
        for nsegs, seed in ROWS_BATCHES:
            rows, tiles = rows_for(nsegs, seed)
            cases.append(dict(form="copy_rows", nsegs=nsegs, seed=seed, rows=rows, tiles=tiles))
    else:
        raise ValueError(family)
    return cases


def rows_tiles(segs, rows):
    """The batch's tile count (rows_map.hpp rows_tiles_per_row)."""
    return rows * sum(-(-(n // 16 + 1) // 64) for (_, _, n, _, _) in segs)


def rows_for(nsegs, seed):
    """The fewest rows at which the rows_case batch has at least 3 G0 + 1 tiles and no multiple of 8 of them (so no
    multiple of either G): the last pass is uneven."""
    from tests.test_group import rows_case
    per_row = rows_tiles(rows_case(nsegs, 1, seed)[0], 1)
    assert per_row % 8, (nsegs, seed)
    rows = -(-(3 * G0 + 1) // per_row)
    while (rows * per_row) % 8 == 0:
        rows += 1
    return rows, rows * per_row


# ------------------------------------------------------------------------------------------------- in the child
def _run_pair(rng):
    import torch

    import dccl_amd
    ran, bad, data = 0, [], {}
    for case in plan("pair"):
        dt, n, roff, soff = case["dt"], case["count"], case["roff"], case["soff"]
        key = (dt, case["shape"], n)
        if key not in data:
            data.clear()  # cases of one key are consecutive
            op = int(rng.integers(0, 4))
            s, r = rand_inputs(rng, dt, n)
            data[key] = (op, s, r, expected(s, r, dt, op), expected(r, r, dt, op))
        op, s, r, want, want_self = data[key]
        nb = n * esz_of(dt)
        td, pd = dev_bytes(r, roff)
        if soff is None:  # send == recv
            rc = dccl_amd.local_reduce(pd, pd, dt, n, op, 0)
            want, src_ok = want_self, True
        else:
            ts, ps = dev_bytes(s, soff)
            before = ts.clone()
            rc = dccl_amd.local_reduce(ps, pd, dt, n, op, 0)
            src_ok = torch.equal(ts, before)
        torch.cuda.synchronize()
        whole = td.cpu().numpy()
        got = whole[roff:roff + nb].copy().view(r.dtype)
        if not (rc == 0 and src_ok and fp_equal(got, want, dt) and not whole[:roff].any()
                and not whole[roff + nb:].any()):
            where = np.flatnonzero(got.view(np.uint8) != want.view(np.uint8))[:4].tolist() if rc == 0 else []
            bad.append((case, op, rc, src_ok, where))
        ran += 1
    return ran, bad


def _run_premul(rng):
    import torch

    import dccl_amd
    from tests.test_direct import chain_expected
    from tests.test_premul import Scalar, premul, scalars_of
    ran, bad, data = 0, [], {}
    scalars = {(dt, si, res): Scalar(scalars_of(dt)[si], res) for dt in ALL_DTS for si in range(2) for res in range(2)}
    for case in plan("premul"):
        dt, n, roff = case["dt"], case["count"], case["roff"]
        esz = esz_of(dt)
        nb = n * esz
        sc = scalars[(dt, case["scalar"], case["residence"])]
        if case["form"] == "scale":
            key = ("scale", dt, case["shape"], n)
            if key not in data:
                data.clear()
                x = rand_inputs(rng, dt, n)[0]
                data[key] = (x, [premul(x, s, dt) for s in scalars_of(dt)])
            x, wants = data[key]
            want = wants[case["scalar"]]
            ts, ps = dev_bytes(x, case["soff"])
            if case["in_place"]:
                td, pd, before = ts, ps, None
            else:
                td, pd = dev_bytes(np.zeros_like(x), roff)
                before = ts.clone()
            rc = dccl_amd.local_scale(ps, pd, dt, n, sc.ptr, case["residence"])
            torch.cuda.synchronize()
            src_ok = before is None or torch.equal(ts, before)
        else:
            k = case["k"]
            key = ("chain", dt, case["shape"], n, k)
            if key not in data:
                data.clear()
                arrs = [rand_inputs(rng, dt, n)[0] for _ in range(k + 1)]
                s = scalars_of(dt)[case["scalar"]]
                data[key] = (arrs, chain_expected([premul(a, s, dt) for a in arrs[:k]], premul(arrs[k], s, dt), dt, 0))
            arrs, want = data[key]
            holders = [dev_bytes(a, o) for a, o in zip(arrs, case["offs"])]
            before = [h[0].clone() for h in holders[:k]] + ([] if case["in_place"] else [holders[k][0].clone()])
            if case["in_place"]:
                td, pd = holders[k]
            else:
                td, pd = dev_bytes(np.zeros_like(arrs[k]), roff)
            rc = dccl_amd.local_reduce_chain_premul([h[1] for h in holders[:k]], holders[k][1], pd, dt, n, sc.ptr,
                                                    case["residence"])
            torch.cuda.synchronize()
            src_ok = all(torch.equal(h[0], b) for h, b in zip(holders, before))
        whole = td.cpu().numpy()
        got = whole[roff:roff + nb].copy().view(want.dtype)
        if not (rc == 0 and src_ok and fp_equal(got, want, dt) and not whole[:roff].any()
                and not whole[roff + nb:].any()):
            where = np.flatnonzero(got.view(np.uint8) != want.view(np.uint8))[:4].tolist() if rc == 0 else []
            bad.append((case, rc, src_ok, where))
        ran += 1
    return ran, bad


def _run_copies(rng):
    import torch

    import dccl_amd
    from tests.test_group import rows_case, rows_expected
    ran, bad = 0, []
    for case in plan("copies"):
        if case["form"] == "copy_multi":
            nb, soff, doff, npairs = case["nbytes"], case["soff"], case["doff"], case["npairs"]
            src = [rng.integers(0, 256, nb + 64, dtype=np.uint8) for _ in range(npairs)]
            t_src = [torch.from_numpy(s).cuda() for s in src]
            t_dst = [torch.zeros(nb + 64, dtype=torch.uint8, device="cuda") for _ in range(npairs)]
            assert all(t.data_ptr() % 256 == 0 for t in t_src + t_dst)
            torch.cuda.synchronize()
            rc = dccl_amd.copy_multi([t.data_ptr() + soff for t in t_src], [t.data_ptr() + doff for t in t_dst], nb)
            torch.cuda.synchronize()
            ok = rc == 0
            for s, ts, td in zip(src, t_src, t_dst):
                d = td.cpu().numpy()
                ok = ok and d[doff:doff + nb].tobytes() == s[soff:soff + nb].tobytes()
                ok = ok and not d[:doff].any() and not d[doff + nb:].any() and ts.cpu().numpy().tobytes() == s.tobytes()
        else:
            segs, s_len, d_len = rows_case(case["nsegs"], case["rows"], case["seed"])
            src = rng.integers(0, 256, s_len, dtype=np.uint8)
            dst = rng.integers(0, 256, d_len, dtype=np.uint8)
            t_src, t_dst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
            assert t_src.data_ptr() % 256 == 0 and t_dst.data_ptr() % 256 == 0
            torch.cuda.synchronize()
            rc = dccl_amd.copy_rows_multi([(t_src.data_ptr() + s, t_dst.data_ptr() + q, n, ss, ds)
                                           for (s, q, n, ss, ds) in segs], case["rows"])
            torch.cuda.synchronize()
            want = rows_expected(segs, case["rows"], src, dst)  # the guard bands around every row included
            ok = rc == 0 and t_dst.cpu().numpy().tobytes() == want.tobytes()
            ok = ok and t_src.cpu().numpy().tobytes() == src.tobytes()
        if not ok:
            bad.append((case, rc))
        ran += 1
    return ran, bad


def _run_collective(rng):
    """One in-process direct all-reduce, W = 4, fp32 Sum, chunks of 4099 * 5 elements (81 tiles): the chain and the
    gather copy both stride inside a real call.  In place and out of place."""
    import torch

    from tests.test_collectives import _expected_allreduce, run_ranks
    W, dt, op = 4, 7, 0
    n = 4 * 4099 * 5
    assert os.environ.get("DCCL_ALLREDUCE_ALGORITHM", "") == ""  # the default: the direct collectives
    inputs = [rand_inputs(rng, dt, n)[0] for _ in range(W)]
    want = _expected_allreduce(inputs, dt, op)
    ran, bad = 0, []
    for in_place in (True, False):
        def body(comm, r):
            st = torch.cuda.Stream()
            send = torch.from_numpy(inputs[r].view(np.uint8).copy()).cuda()
            recv = send if in_place else torch.zeros_like(send)
            torch.cuda.synchronize()
            rc = comm.all_reduce(send.data_ptr(), recv.data_ptr(), n, dt, op, st.cuda_stream)
            st.synchronize()
            return rc, recv.cpu().numpy().view(np.float32), send.cpu().numpy().view(np.float32)

        out = run_ranks(W, body)
        for r, (rc, got, src) in enumerate(out):
            ok = rc == 0 and fp_equal(got, want[r], dt) and (in_place or src.tobytes() == inputs[r].tobytes())
            if not ok:
                bad.append((in_place, r, rc))
        ran += 1
    return ran, bad


def run_family(family):
    """In the child: every case of the family on the GPU; returns (cases run, failures)."""
    import torch
    torch.cuda.set_device(0)
    rng = np.random.default_rng(8000 + (FAMILIES + ["collective"]).index(family))
    if family in ("classes", "windows", "routed"):
        ran, bad, pairs_k, pairs_size = forms.run_cases(plan(family), rng, check_sources=True)
        # the plan really met every (k, dtype) and (dtype, shape) pair
        assert {(form, k, dt) for form, ks in KS.items() for k in ks for dt in DTS} == pairs_k
        assert {(s, dt) for s in SHAPES for dt in DTS} == pairs_size
        return ran, bad
    return {"pair": _run_pair, "premul": _run_premul, "copies": _run_copies, "collective": _run_collective}[family](rng)


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import dccl_amd
assert dccl_amd.lib.dccl_max_grid_test() == int(sys.argv[3]), "the grid clamp is not live in this process"
assert dccl_amd.lib.dccl_caps_test_shift() == int(sys.argv[4]), "the size scale is not live in this process"
from tests import test_gpu_grid_stride_small as stride
ran, bad = stride.run_family(sys.argv[2])
for b in bad[:8]:
    print("BAD", b)
print("GRID", dccl_amd.lib.dccl_max_grid_test(), "SHIFT", dccl_amd.lib.dccl_caps_test_shift())
print("RAN", ran)
sys.exit(1 if bad else 0)
"""


def _child(family, G, shift):
    env = {**os.environ, "DCCL_MAX_GRID_TEST": str(G), "DCCL_CAPS_TEST_SHIFT": str(shift), "PYTHONPATH": ROOT}
    env.pop("DCCL_ALLREDUCE_ALGORITHM", None)  # the collective child runs the default whatever an earlier test left
    t0 = time.monotonic()
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, family, str(G), str(shift)], env=env, capture_output=True,
                       text=True, timeout=180)
    print(f"{family} G={G} shift={shift}: child wall time {time.monotonic() - t0:.1f} s")
    print(p.stdout[-3000:])
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert f"GRID {G} SHIFT {shift}" in p.stdout.splitlines()
    assert f"RAN {EXPECTED_CASES[family]}" in p.stdout.splitlines(), p.stdout[-500:]


def check_plan():
    """No GPU work (tests/test_tile_maps.py runs it in the CPU suite): each family's plan has the stated number of
    cases, and every planned case has at least 2 G0 + 1 tiles (a third pass at G = 104, and so at G = 8), computed
    from count, dtype and destination offset; the row batches at least 3 G0 + 1 and no multiple of either G."""
    for family in FAMILIES:
        cases = plan(family)
        assert len(cases) == EXPECTED_CASES[family], (family, len(cases))
        for c in cases:
            tiles = c["tiles"] if "tiles" in c else tiles_of(c["count"], c["dt"], c["roff"])
            assert tiles >= 2 * G0 + 1, c
            if c["form"] == "copy_rows":
                assert tiles >= 3 * G0 + 1 and tiles % G0 and tiles % 8, c
    # the shapes are the stated vectors whatever the destination's offset
    for dt in ALL_DTS:
        esz = esz_of(dt)
        for nvec, tail in SHAPES:
            for doff in (0, esz, 1, 33 + esz // 2):
                n = count_for((nvec, tail), dt, doff)
                assert tiles_of(n, dt, doff) == -(-nvec // 64), (dt, nvec, doff)
                assert n * esz < 330 * 1024
    assert [-(-s[0] // 64) for s in SHAPES] == [3 * G0, 3 * G0 + 1, 2 * G0 + G0 // 2 + 1, 3 * G0, 2 * G0 + 6]


def test_knobs_are_off_in_the_suite_process(gpu):
    import dccl_amd
    assert "DCCL_MAX_GRID_TEST" not in os.environ and "DCCL_CAPS_TEST_SHIFT" not in os.environ
    assert dccl_amd.lib.dccl_max_grid_test() == 0
    assert dccl_amd.lib.dccl_caps_test_shift() == 0


@pytest.mark.parametrize("G,shift", SETTINGS)
@pytest.mark.parametrize("family", FAMILIES)
def test_grid_stride_passes_at_small_sizes(gpu, family, G, shift):
    """pair (dccl_local_reduce, all ten dtypes): aligned, in place with send == recv, send 16 B off the
    destination's lines (StraddleCfg), send at other element phases and at byte phases (the shifted kernel, both
    load policies), destination off element alignment at offsets 1 and 33 + sizeof(T) / 2
    (reduce_unaligned_kernel); each with the destination on its 128-B line and one element in (head scalars).
    classes: the in-phase, straddle and phased k-way (k = 2..8) and chain (k = 1..8) launches, the chain in place
    and with a separate own.  windows: a destination that is not element-aligned (reduce_windows_kernel from
    k = 3, the round-3 forms below), sources at phase 0, phase 4, mixed byte phases and one off phase, own in
    place, at phase 0 and at 4.  routed: an element-aligned destination with sources at other element phases, at
    byte phase 1 and with one off phase (the phased kernels, or reduce_windows_kernel where the size routes them
    there).  In these three every dtype wider than a byte meets every k and every shape.  premul:
    dccl_local_scale in place, at the same phase, at another phase and with the destination 1 B off;
    dccl_local_reduce_chain_premul in phase, at mixed phases and off element alignment, k = 1..8; all ten dtypes,
    both scalar residences, the scalars of scalars_of.  copies: dccl_copy_multi with 1, 3 and 8 pairs at the
    byte-offset pairs of test_copy_multi; dccl_copy_rows_multi with rows_case batches of 1, 5 and 32 segments."""
    _child(family, G, shift)


def test_direct_all_reduce_strides_inside_a_real_call(gpu):
    _child("collective", 8, 0)
