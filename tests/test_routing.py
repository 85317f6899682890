"""Where the operands of a k-way or chain combine lie and which launch takes them (dccl_amd/csrc/routing.hpp), on
the CPU: routing.hpp is host-only C++, compiled here with g++ into a small harness that reads one placement per
line and prints route(): the chosen launch, the destination's split and the operands' phases.  The expected
values are the rules of reduce_multi_typed / reduce_chain_typed (local_reduce.hip before the two became one
function), restated below in Python; the grid is exhaustive over both orders, 1..8 sources, every element size,
destination offsets on and off element, 16-B and 128-B alignment, the source patterns that select a launch, and
counts from 0 to both sides of the 48 and 96 MiB thresholds of caps::phased_via_windows."""
import itertools
import subprocess

import pytest

from tests.test_caps import CSRC

HARNESS = r"""
#include <cstdio>
#include "routing.hpp"
using namespace dccl_amd;
int main() {
    int chain, nsend;
    unsigned long long esz, count, dst, own, s[8];
    while (std::scanf("%d %d %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu", &chain, &nsend, &esz, &count,
                      &dst, &own, &s[0], &s[1], &s[2], &s[3], &s[4], &s[5], &s[6], &s[7]) == 14) {
        const void* sends[8];
        for (int k = 0; k < 8; ++k) sends[k] = reinterpret_cast<const void*>(uintptr_t(s[k]));
        const Routed r = route(chain != 0, nsend, size_t(esz), sends, reinterpret_cast<const void*>(uintptr_t(own)),
                               reinterpret_cast<const void*>(uintptr_t(dst)), size_t(count), 128, size_t(count * esz));
        std::printf("%d %zu %zu %zu", int(r.route), r.sp.head, r.sp.nvec, r.sp.tail);
        for (int k = 0; k < 9; ++k) std::printf(" %u", r.ph.p[k]);
        std::printf("\n");
        // the classifier alone, as the pre-multiplied and wide chains use it
        const Placement c = classify(sends, nsend, reinterpret_cast<const void*>(uintptr_t(own)),
                                     reinterpret_cast<const void*>(uintptr_t(dst)), size_t(esz));
        std::printf("%d %d\n", int(c.elem_ok), int(c.in_phase()));
    }
}
"""

PAIR, WINDOWS_DST_OFF, WINDOWS_VIA_CAPS, PHASED, STRADDLE, IN_PHASE = range(6)
MIB = 1 << 20
ALIGN = 128
DST_BASE, OWN_BASE, SRC_BASE, SRC_STRIDE = 0x10000000, 0x90000000, 0x20000000, 0x01000000
PATTERNS = ["in_phase_on_grid", "in_phase_off_grid", "one_off_by_esz", "one_off_by_1", "own_only_off", "in_place"]


def phased_via_windows(chain, k, nbytes, dst16):
    """caps.hpp, frozen by tests/test_caps.py."""
    if nbytes >= 96 * MIB:
        return (4 if chain else 3) <= k <= (7 if chain else 5)
    return dst16 and (3 if chain else 4) <= k <= 8 and 48 * MIB <= nbytes < 96 * MIB


def split(dst, count, esz):
    v = 16 // esz
    head = min(((ALIGN - dst % ALIGN) % ALIGN) // esz, count)
    nvec = (count - head) // v
    return head, nvec, count - head - nvec * v


def parent_route(chain, nsend, esz, sends, own, dst, count):
    """(route, split, phases): the rules of reduce_multi_typed (chain false: own is dst) and reduce_chain_typed."""
    none, zeros = (0, 0, 0), [0] * 9
    nbytes = count * esz

    def phases(off):
        ph = [(s + off) % 16 for s in sends] + ([(own + off) % 16] if chain else [])
        return ph + [0] * (9 - len(ph))

    if not chain:
        if nsend == 1:
            return PAIR, none, zeros
        vec_ok = dst % esz == 0 and all((s ^ dst) & 15 == 0 for s in sends)
        if dst % esz:
            return WINDOWS_DST_OFF, none, phases(0)
        if not vec_ok:
            if esz > 1 and phased_via_windows(False, nsend, nbytes, dst % 16 == 0):
                return WINDOWS_VIA_CAPS, none, phases(0)
            sp = split(dst, count, esz)
            return PHASED, sp, phases(sp[0] * esz)
    else:
        if nsend == 1 and own == dst:
            return PAIR, none, zeros
        src_off = any((s ^ dst) & 15 for s in sends)
        vec_ok = dst % esz == 0 and (dst ^ own) & 15 == 0 and not src_off
        if dst % esz:
            return WINDOWS_DST_OFF, none, phases(0)
        if not vec_ok:
            if esz > 1 and src_off and phased_via_windows(True, nsend, nbytes, dst % 16 == 0):
                return WINDOWS_VIA_CAPS, none, phases(0)
            sp = split(dst, count, esz)
            return PHASED, sp, phases(sp[0] * esz)
    sp = split(dst, count, esz)
    straddles = any((s + sp[0] * esz) % 128 for s in sends)
    return (STRADDLE if straddles else IN_PHASE), sp, zeros


def cases():
    for chain, nsend, esz in itertools.product((0, 1), range(1, 9), (1, 2, 4, 8)):
        counts = [0, 1, max(16 // esz - 1, 1)] + [b // esz + d for b in (48 * MIB, 96 * MIB) for d in (-1, 0)]
        for doff, pattern, count in itertools.product((0, 1, esz, 16, 128 + esz), PATTERNS, counts):
            dst = DST_BASE + doff
            soffs = [doff] * nsend
            own = OWN_BASE + doff + 32 if chain else dst  # a separate own in the destination's phase
            if pattern == "in_phase_off_grid":
                soffs = [doff + 16 * (1 + k % 7) for k in range(nsend)]
            elif pattern == "one_off_by_esz":
                soffs[nsend - 1] += esz
            elif pattern == "one_off_by_1":
                soffs[0] += 1
            elif pattern == "own_only_off" and chain:
                own += esz
            elif pattern == "in_place":
                own = dst
            sends = [SRC_BASE + k * SRC_STRIDE + o for k, o in enumerate(soffs)]
            yield chain, nsend, esz, count, dst, own, sends


@pytest.fixture(scope="module")
def routed(tmp_path_factory):
    d = tmp_path_factory.mktemp("routing")
    src, exe = d / "route_dump.cpp", d / "route_dump"
    src.write_text(HARNESS)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}", str(src), "-o", str(exe)],
                   check=True)
    lines = [" ".join(map(str, [chain, nsend, esz, count, dst, own] + sends + [0] * (8 - nsend)))
             for chain, nsend, esz, count, dst, own, sends in cases()]
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout
    rows = [list(map(int, l.split())) for l in out.splitlines()]
    assert len(rows) == 2 * len(lines)
    return rows


def test_route_is_the_parent_rules_on_the_whole_grid(routed):
    seen = set()
    for case, row in zip(cases(), routed[0::2]):
        chain, nsend, esz, count, dst, own, sends = case
        route, sp, ph = parent_route(chain, nsend, esz, sends, own, dst, count)
        assert row == [route, *sp, *ph], (case, row)
        seen.add((chain, route))
    assert seen == {(c, r) for c in (0, 1) for r in range(6)}  # every launch of both orders is reached


def test_differences_between_the_two_orders_survive(routed):
    """The chain asks for sources off phase before phased_via_windows, and takes the pair short cut only in place."""
    got = {tuple(case[:6]) + tuple(case[6]): row[0] for case, row in zip(cases(), routed[0::2])}
    n96 = 96 * MIB // 4

    def addr(chain, nsend, own_off=0, src_off=0, in_place=False):
        dst = DST_BASE
        own = dst if in_place or not chain else OWN_BASE + 32 + own_off
        sends = [SRC_BASE + k * SRC_STRIDE for k in range(nsend)]
        sends[nsend - 1] += src_off
        return (chain, nsend, 4, n96, dst, own, *sends)

    assert got[addr(1, 5, own_off=4)] == PHASED              # own alone off phase keeps the phased kernels
    assert got[addr(1, 5, src_off=4)] == WINDOWS_VIA_CAPS    # a source off phase: the windows kernel from 96 MiB
    assert got[addr(0, 5, src_off=4)] == WINDOWS_VIA_CAPS
    assert got[addr(0, 1)] == PAIR and got[addr(1, 1, in_place=True)] == PAIR
    assert got[addr(1, 1)] == IN_PHASE                       # one source, a separate own: the chain kernel


def test_classifier_of_the_extended_chains(routed):
    """classify(): elem_ok and in_phase as chain_forms.hpp's launch_chain_form reads them."""
    for case, (elem_ok, in_phase) in zip(cases(), routed[1::2]):
        chain, nsend, esz, count, dst, own, sends = case
        ops = [dst, own] + sends
        assert elem_ok == int(all(a % esz == 0 for a in ops)), case
        assert in_phase == int(all((a ^ dst) & 15 == 0 for a in ops)), case
