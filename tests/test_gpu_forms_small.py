"""GPU parity of the combine forms that only the operand size selects, at small sizes.

Three parts of the hot path are chosen by bytes per operand alone (dccl_amd/csrc/caps.hpp): the tuned and
mid-size forms of reduce_windows_kernel (from 96 and 48 MiB: the loads-first tile, the group and run-of-4 tile
orders, the routing of element-aligned destinations away from the phased kernels) and rows 1-3 of caps::kWaves
(from 24, 48 and 96 MiB: the larger dynamic-LDS requests of the in-phase, straddle and phased launches).  With
DCCL_CAPS_TEST_SHIFT=10 (dispatch.hpp caps_bytes, read once per process) an operand of n bytes selects the forms
of one of n MiB per KiB (n << 10), so the mid forms start at 48 KiB and the tuned forms at 96 KiB = 96 tiles of
1 KiB = three run-of-4 spans of 32 blocks: every partial tile, dead lane, partial group and element tail of
those forms is reached with operands of about 100 KiB.

Each family runs in one fresh child process with the shift in its environment.  The child first asserts that
dccl_caps_test_shift() is 10 (a child that silently ran the small-size forms would prove nothing), runs every
case of plan(family), counts them and prints the count; the parent asserts the count against the family's own
product.  Every case: operands of raw bit patterns (NaN, infinity, denormals: rand_inputs), the result bit for
bit (any NaN equals any NaN, fp_equal) against oracle.combine applied in the kernel's documented order (k-way
sequential; chain in the ring's order), and every guard byte before and after the destination still zero."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import oracle
from tests.test_gpu_parity import dev_bytes, expected, rand_inputs
from tests.test_oracle import fp_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFT = 10
KIB = 1 << 10
DTS = [2, 3, 4, 5, 6, 7, 8, 9]  # every dtype wider than a byte
SLOTS = 8                        # k cycles over SLOTS slots, so every shape meets every dtype

# (nvec, tail): count = nvec * V + tail elements, V = 16 / sizeof(T); tail "V-1" is V - 1 elements.
TUNED = [(6144, 0),               # 96 tiles exactly
         (6145, 0),               # one live lane in the last tile; grid 104, partial run-of-4 group of 8
         (64 * 104 + 63, "V-1"),  # grid 112, partial group of 16
         (64 * 112 + 33, 1),      # grid 120, partial group of 24
         (64 * 127 + 1, 0),       # grid 128, no partial group
         (64 * 200 + 7, "V-1")]
MID = [(3072, 0), (3073, 0), (64 * 64, 1), (64 * 64 + 63, "V-1"), (64 * 95 + 62, "V-1")]
BOUNDARY = [48 * KIB, 96 * KIB]   # bytes = this - sizeof(T): the form just below each threshold
SHAPES = [("tuned", s) for s in TUNED] + [("mid", s) for s in MID] + [("below", b) for b in BOUNDARY]
BYTE_PHASES = [0, 1, 4, 7, 8, 12, 15]

WINDOWS_SRC = ["phase0", "phase4", "mixed", "one_off"]
WINDOWS_OWN = ["in_place", "own0", "own4"]
ROUTED_SRC = ["elem_off", "byte1", "one_off"]
ROUTED_CHAIN = [(s, o) for s in ROUTED_SRC for o in ("in_place", "own_in_phase")] + [("in_phase", "own_only_off")]
ROW_BYTES = [24 * KIB, 48 * KIB, 96 * KIB]
ROW_CLASSES = ["in_phase", "straddle", "phased"]
ROW_K = {"multi": [2, 5, 8], "chain": [1, 4, 8]}

FAMILY_KS = {"windows_kway": {"multi": range(2, 9)}, "windows_chain": {"chain": range(1, 9)},
             "routed": {"multi": range(2, 7), "chain": range(3, 9)}, "size_rows": ROW_K}
# cases per family: 13 shapes x 8 slots meet every dtype 13 times; the six 4- and 8-byte dtypes have two
# misaligned destination offsets, the two 16-bit ones one (33 + 1 is a multiple of 2)
_ROFFS = len(SHAPES) * (6 * 2 + 2 * 1)
EXPECTED_CASES = {
    "windows_kway": _ROFFS * len(WINDOWS_SRC),
    "windows_chain": _ROFFS * len(WINDOWS_SRC) * len(WINDOWS_OWN),
    "routed": SLOTS * len(SHAPES) * 2 * (len(ROUTED_SRC) + len(ROUTED_CHAIN)),
    "size_rows": 2 * 3 * len(ROW_BYTES) * len(ROW_CLASSES) * 3,
    "windows_first_sweep": 2 * 2 * 16,
}
# windows_first_sweep: the loads-first window tile (tuned off-phase form at K = 5) with source 0, and the chain's
# own, at every byte phase 0..15; the other sources at phase 4, so every case is the off-phase class
SWEEP_SHAPE = ("tuned", TUNED[1])
SWEEP_K = 5
SWEEP_DTS = [7, 9]


def esz_of(dt):
    return int(np.dtype(oracle.NP_DTYPES[dt]).itemsize)


def count_of(shape, dt):
    kind, s = shape
    esz = esz_of(dt)
    if kind == "below":
        return (s - esz) // esz
    nvec, tail = s
    v = 16 // esz
    return nvec * v + (v - 1 if tail == "V-1" else tail)


def plan(family):
    """The cases of a family, without data: dicts of form, k, dt, shape, count and the placement names.  The
    dtype cycles with the slot and the shape, so every (k, dtype) and every (dtype, size) pair occurs."""
    cases = []
    if family == "windows_first_sweep":
        for form in ("multi", "chain"):
            for dt in SWEEP_DTS:
                for phase in range(16):
                    cases.append(dict(form=form, k=SWEEP_K, dt=dt, shape=SWEEP_SHAPE, count=count_of(SWEEP_SHAPE, dt),
                                      roff=1, src="sweep", own="own_sweep" if form == "chain" else "none",
                                      phase=phase))
        return cases
    if family == "size_rows":
        for form, ks in ROW_K.items():
            for ki, k in enumerate(ks):
                for si, nb in enumerate(ROW_BYTES):
                    for ci, cls in enumerate(ROW_CLASSES):
                        for m in range(3):  # ci + 3 m runs over 0..8: every dtype at every (k, size)
                            dt = DTS[(ki + si + ci + 3 * m) % 8]
                            esz = esz_of(dt)
                            v = 16 // esz
                            # head scalars up to the destination's 128-B line, nb / 16 + 5 vectors (a partial
                            # last tile of 5 lanes, sp.nvec * 16 just above nb), V - 1 tail scalars
                            count = (128 - esz) // esz + (nb // 16 + 5) * v + (v - 1)
                            cases.append(dict(form=form, k=k, dt=dt, shape=("row", nb), count=count, roff=esz,
                                              src=cls, own="in_place"))
        return cases
    for form, ks in FAMILY_KS[family].items():
        ks = list(ks)
        for j in range(SLOTS):
            k = ks[j % len(ks)]
            for si, shape in enumerate(SHAPES):
                dt = DTS[(j + si) % 8]
                esz = esz_of(dt)
                if family == "routed":
                    roffs = [0, esz]  # the destination 16-B aligned, and element-aligned only
                    placements = [(s, "none") for s in ROUTED_SRC] if form == "multi" else ROUTED_CHAIN
                else:
                    roffs = [1] + ([33 + esz // 2] if (33 + esz // 2) % esz else [])
                    placements = [(s, o) for s in WINDOWS_SRC for o in (WINDOWS_OWN if form == "chain" else ["none"])]
                for roff in roffs:
                    for src, own in placements:
                        cases.append(dict(form=form, k=k, dt=dt, shape=shape, count=count_of(shape, dt), roff=roff,
                                          src=src, own=own, slot=j))
    return cases


def source_offsets(rng, case):
    """Byte offset of each source inside its own 256-B aligned allocation."""
    k, esz, roff, src = case["k"], esz_of(case["dt"]), case["roff"], case["src"]
    lanes = [16 * j for j in range(k)]
    if src == "phase0":
        ph = [0] * k
    elif src == "phase4":
        ph = [4] * k
    elif src == "mixed":  # byte phases, at least one non-zero
        ph = [int(rng.choice(BYTE_PHASES)) for _ in range(k)]
        if not any(ph):
            ph[int(rng.integers(k))] = int(rng.choice(BYTE_PHASES[1:]))
    elif src == "sweep":  # source 0 at the case's byte phase, the others at phase 4
        ph = [case["phase"]] + [4] * (k - 1)
    elif src == "byte1":  # not element-aligned
        ph = [1] * k
    elif src == "in_phase":  # the destination's own 16-B phase, on its 128-B lines
        return [roff] * k
    elif src == "straddle":  # the destination's 16-B phase, off its lines
        return [roff + 16 * (1 + j % 7) for j in range(k)]
    elif src == "phased":  # element-aligned, another 16-B phase
        return [roff + esz + 16 * j for j in range(k)]
    elif src == "elem_off":  # element-aligned phases other than the destination's
        others = [p for p in range(0, 16, esz) if p != roff % 16]
        ph = [int(rng.choice(others)) for _ in range(k)]
    else:  # one_off: exactly one source off the others' phase
        assert src == "one_off"
        base = roff % 16 if case["roff"] % esz == 0 else 0  # routed: the destination's phase; windows: phase 0
        ph = [base] * k
        choices = [p for p in (BYTE_PHASES if roff % esz else range(0, 16, esz)) if p != base]
        ph[int(rng.integers(k))] = int(rng.choice(choices))
    return [a + b for a, b in zip(lanes, ph)]


def run_cases(cases, rng, check_sources=False):
    """In a child: every case of a plan on the GPU; returns (cases run, failures, the (form, k, dtype) and the
    (shape, dtype) pairs met).  tests/test_gpu_grid_stride_small.py runs its k-way and chain plans through it too,
    with check_sources: every source allocation is compared with a device copy taken before the launch."""
    import torch

    import dccl_amd
    torch.cuda.set_device(0)
    ran, bad = 0, []
    pairs_k, pairs_size = set(), set()
    data = {}  # (form, slot / k, shape, dt) -> operands and both references, computed once and left unchanged

    def operands(case):
        key = (case["form"], case.get("slot", case["k"]), case["shape"], case["dt"])
        if key not in data:
            data.clear()  # cases of one key are consecutive
            k, dt, n = case["k"], case["dt"], case["count"]
            op = int(rng.integers(0, 4))
            sends = [rand_inputs(rng, dt, n)[0] for _ in range(k)]
            r = rand_inputs(rng, dt, n)[1]
            if case["form"] == "multi":  # recv = op(...op(op(recv, s0), s1)..., s{k-1})
                want = r
                for x in sends:
                    want = expected(x, want, dt, op)
            else:  # dst = op(own, op(s{k-1}, ... op(s1, s0)))
                acc = sends[0]
                for x in sends[1:]:
                    acc = expected(acc, x, dt, op)
                want = expected(acc, r, dt, op)
            data[key] = (op, sends, r, want)
        return data[key]

    for case in cases:
        form, k, dt, n, roff = case["form"], case["k"], case["dt"], case["count"], case["roff"]
        esz = esz_of(dt)
        op, sends, r, want = operands(case)
        holders = [dev_bytes(x, o) for x, o in zip(sends, source_offsets(rng, case))]
        sptrs = [h[1] for h in holders]
        before = [h[0].clone() for h in holders] if check_sources else []
        own = case["own"]
        if own in ("none", "in_place"):
            td, pd = dev_bytes(r, roff)
            po = pd
        else:  # a separate own; the destination starts as zeros
            ooff = {"own0": 0, "own4": 4, "own_in_phase": roff % 16 + 32, "own_only_off": (roff + esz) % 16 + 32,
                    "own_sweep": case.get("phase", 0)}[own]
            to, po = dev_bytes(r, ooff)
            td, pd = dev_bytes(np.zeros_like(r), roff)
        if form == "multi":
            rc = dccl_amd.local_reduce_multi(sptrs, pd, dt, n, op, 0)
        else:
            rc = dccl_amd.local_reduce_chain(sptrs, po, pd, dt, n, op, 0)
        torch.cuda.synchronize()
        whole = td.cpu().numpy()
        nb = n * esz
        got = whole[roff:roff + nb].copy().view(r.dtype)
        ok = rc == 0 and fp_equal(got, want, dt) and not whole[:roff].any() and not whole[roff + nb:].any()
        ok = ok and all(torch.equal(h[0], b) for h, b in zip(holders, before))
        if check_sources and own not in ("none", "in_place"):
            ok = ok and to.cpu().numpy()[ooff:ooff + nb].tobytes() == r.tobytes()
        if not ok:
            where = np.flatnonzero(got.view(np.uint8) != want.view(np.uint8))[:4].tolist() if rc == 0 else []
            bad.append((case, op, rc, where))
        ran += 1
        pairs_k.add((form, k, dt))
        pairs_size.add((case["shape"], dt))
    return ran, bad, pairs_k, pairs_size


def run_family(family):
    """In the child: every case of plan(family) on the GPU; returns (cases run, failures)."""
    if family == "windows_first_sweep":
        ran, bad, pairs_k, _ = run_cases(plan(family), np.random.default_rng(7100))
        assert pairs_k == {(form, SWEEP_K, dt) for form in ("multi", "chain") for dt in SWEEP_DTS}
        return ran, bad
    rng = np.random.default_rng(7000 + sorted(FAMILY_KS).index(family))
    ran, bad, pairs_k, pairs_size = run_cases(plan(family), rng)
    # the plan really met every (k, dtype) and (dtype, size) pair
    for form, ks in FAMILY_KS[family].items():
        assert {(form, k, dt) for k in ks for dt in DTS} <= pairs_k, "a (k, dtype) pair is missing"
    shapes = [("row", b) for b in ROW_BYTES] if family == "size_rows" else SHAPES
    assert {(s, dt) for s in shapes for dt in DTS} == pairs_size, "a (dtype, size) pair is missing"
    return ran, bad


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import dccl_amd
assert dccl_amd.lib.dccl_caps_test_shift() == int(sys.argv[3]), "the size scale is not live in this process"
from tests import test_gpu_forms_small as forms
ran, bad = forms.run_family(sys.argv[2])
for b in bad[:8]:
    print("BAD", b)
print("SHIFT", dccl_amd.lib.dccl_caps_test_shift())
print("RAN", ran)
sys.exit(1 if bad else 0)
"""


def test_plan_is_the_stated_product():
    """No GPU work: each family's plan has the stated number of cases, the shapes are the stated bytes."""
    for family, want in EXPECTED_CASES.items():
        assert len(plan(family)) == want, family
    for dt in DTS:
        esz = esz_of(dt)
        for kind, s in SHAPES:
            nb = count_of((kind, s), dt) * esz
            if kind == "tuned":
                assert nb >= 96 * KIB
            elif kind == "mid":
                assert 48 * KIB <= nb < 96 * KIB
            else:
                assert nb == s - esz
    assert count_of(("tuned", TUNED[0]), 7) * 4 == 96 * KIB and count_of(("mid", MID[0]), 6) * 2 == 48 * KIB


def test_shift_is_zero_in_the_suite_process(gpu):
    import dccl_amd
    assert "DCCL_CAPS_TEST_SHIFT" not in os.environ
    assert dccl_amd.lib.dccl_caps_test_shift() == 0


@pytest.mark.parametrize("family", ["windows_kway", "windows_chain", "routed", "size_rows", "windows_first_sweep"])
def test_size_selected_forms_at_small_sizes(gpu, family):
    """windows_kway / windows_chain: a destination that is not element-aligned (offset 1, and 33 + sizeof(T) / 2),
    sources all at 16-B phase 0 (the in-phase class), all at phase 4, at mixed byte phases and with exactly one
    off phase; the chain in place and with a separate own at phase 0 and 4; k-way k = 2..8, chain k = 1..8; the
    six tuned and five mid-size shapes above and the size just below each threshold.  routed: an element-aligned
    destination (16-B aligned and not) with sources at other element-aligned phases, at byte phase 1, and with one
    source off phase, k-way k = 2..6 and chain k = 3..8 (both sides of the routed ranges 3..5 and 4..7), and the
    chain whose own alone is off phase (it keeps the phased kernels).  size_rows: the in-phase, straddle and
    phased k-way (k = 2, 5, 8) and chain (k = 1, 4, 8) launches just above 24, 48 and 96 KiB with head and tail
    scalars and a partial last tile: each carries the larger LDS request of its caps::kWaves row and must return
    0 and the exact result (at 96 KiB the phased k-way k = 5 and chain k = 4 launches are routed to
    reduce_windows_kernel, as at 96 MiB).  windows_first_sweep: the loads-first window tile (k = 5, 6145 vectors,
    destination at offset 1, fp32 and bf16) with source 0, and the chain's separate own, at every byte phase
    0..15 and the other sources at phase 4: the funnel shift at every byte count in that tile."""
    env = {**os.environ, "DCCL_CAPS_TEST_SHIFT": str(SHIFT), "PYTHONPATH": ROOT}
    t0 = time.monotonic()
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, family, str(SHIFT)], env=env, capture_output=True,
                       text=True, timeout=180)
    print(f"{family}: child wall time {time.monotonic() - t0:.1f} s")
    print(p.stdout[-3000:])
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert f"SHIFT {SHIFT}" in p.stdout.splitlines()
    assert f"RAN {EXPECTED_CASES[family]}" in p.stdout.splitlines(), p.stdout[-500:]
