"""Which algorithm runs a collective (dccl_amd/csrc/select.hpp), on the CPU: select.hpp is host-only C++, compiled
here with g++ into a small harness that reads one case per line and prints parse_algo(), select() and slots().  The
expected values are the rules as they stood before the header existed, restated below in Python: the if-chains that
opened ar_run, rs_run, reduce_run, ag_run and bcast_run (dccl_api.cpp) with direct_selected / host_direct_selected
(direct.cpp), grouped_selected, allreduce_algorithm and runs_rabenseifner (dccl_api.cpp).  The grid is the full
product of the 5 collectives, 4 transports, W in {1, 2, 3, 8, 9, 64}, host / device buffers, the 4 sum kinds and 8
values of DCCL_ALLREDUCE_ALGORITHM; combinations the validators reject (host buffers on IPC, a user op on host
buffers, an unknown name) get the answer the run function would have given."""
import itertools
import subprocess

import pytest

from tests.test_caps import CSRC

HARNESS = r"""
#include <cstdio>
#include <cstring>
#include "select.hpp"
using namespace dccl_amd;
int main() {
    int api, transport, device, kind;
    unsigned world;
    char name[64];
    while (std::scanf("%d %d %u %d %d %63s", &api, &transport, &world, &device, &kind, name) == 6) {
        const char* s = std::strcmp(name, "<unset>") == 0 ? nullptr : std::strcmp(name, "<empty>") == 0 ? "" : name;
        const AlgoName a = parse_algo(s);
        const Path p = select(api, Transport(transport), world, device != 0, SumKind(kind), a);
        std::printf("%d %d %zu\n", int(a), int(p), slots(p, world));
    }
}
"""

ALL_REDUCE, REDUCE_SCATTER, REDUCE, ALL_GATHER, BROADCAST = range(5)        # group_plan.hpp Api
THREADS, IPC, RCCL, P2P = range(4)                                          # select.hpp Transport
BUILTIN, PREMUL, WIDE, WIDE_SCALED = range(4)                               # select.hpp SumKind
AUTO, RING_NAME, RAB_NAME, DIRECT_NAME, GROUPED_NAME, UNKNOWN = range(6)    # select.hpp AlgoName
LOCAL, DIRECT, HOST_DIRECT, WIDE_STAGED, GROUPED, RABENSEIFNER, RING = range(7)  # select.hpp Path
WORLDS = (1, 2, 3, 8, 9, 64)
NAMES = (None, "", "auto", "ring", "rabenseifner", "direct", "grouped", "binary_blocks")
DIRECT_MAX_WORLD = 8


# ---- the communicator as the old predicates saw it: ipc, rccl, p2p (RCCL plugs its own p2p in), group
def has_ipc(t):
    return t == IPC


def has_p2p(t):
    return t in (RCCL, P2P)


def has_group(t):
    return t == THREADS


def direct_selected(t, W, a):
    if has_ipc(t):
        return True
    if has_p2p(t) or W > DIRECT_MAX_WORLD:
        return False
    if a is None or a == "":
        return True
    return a in ("auto", "direct")


def host_direct_selected(t, W, a):
    if has_ipc(t) or has_p2p(t) or not has_group(t) or W > DIRECT_MAX_WORLD:
        return False
    if a is None or a == "":
        return True
    return a in ("auto", "direct")


def grouped_selected(t, W, device, a):
    if not device or t != RCCL or W < 2:
        return False
    return a == "grouped"


def allreduce_algorithm(a):
    """The old four-valued enum: "auto" folded into the ring, "grouped" into direct."""
    if a is None or a == "" or a == "ring" or a == "auto":
        return "ring"
    if a == "rabenseifner":
        return "rabenseifner"
    if a in ("direct", "grouped"):
        return "direct"
    return "unknown"


def runs_rabenseifner(api, t, W, device, a):
    if api != ALL_REDUCE or allreduce_algorithm(a) != "rabenseifner" or W <= 1:
        return False
    if device and direct_selected(t, W, a):
        return False
    if not device and host_direct_selected(t, W, a):
        return False
    return True


def parent_path(api, t, W, device, kind, a):
    wide, builtin = kind in (WIDE, WIDE_SCALED), kind == BUILTIN
    if api == ALL_REDUCE:
        if W > 1 and device and direct_selected(t, W, a):
            return DIRECT
        if W > 1 and not device and host_direct_selected(t, W, a):
            return HOST_DIRECT
        if wide:
            return WIDE_STAGED
        if W > 1 and allreduce_algorithm(a) != "rabenseifner" and builtin and grouped_selected(t, W, device, a):
            return GROUPED
        if W == 1:
            return LOCAL  # stage_input, then "if (W == 1) return"
        return RABENSEIFNER if runs_rabenseifner(api, t, W, device, a) else RING
    if api == REDUCE_SCATTER:
        if W > 1 and device and direct_selected(t, W, a):
            return DIRECT
        if W > 1 and not device and host_direct_selected(t, W, a):
            return HOST_DIRECT
        if wide:
            return WIDE_STAGED
        if W > 1 and builtin and grouped_selected(t, W, device, a):
            return GROUPED
        return RING if W > 1 else LOCAL  # "if (W > 1)" around the ring: W == 1 stages and copies out
    if api == REDUCE:
        if W > 1 and device and direct_selected(t, W, a):
            return DIRECT
        if wide:
            return WIDE_STAGED
        return RING if W > 1 else LOCAL  # stage_input, then "if (W == 1) return"
    if W > 1 and device and direct_selected(t, W, a):  # all-gather, broadcast: the form is never looked at
        return DIRECT
    return RING if W > 1 else LOCAL  # one rank: its own copy, and a ring / fan-out that moves nothing


def parent_name(a):
    return {None: AUTO, "": AUTO, "auto": AUTO, "ring": RING_NAME, "rabenseifner": RAB_NAME, "direct": DIRECT_NAME,
            "grouped": GROUPED_NAME}.get(a, UNKNOWN)


def cases():
    return itertools.product(range(5), range(4), WORLDS, (0, 1), range(4), NAMES)


@pytest.fixture(scope="module")
def selected(tmp_path_factory):
    d = tmp_path_factory.mktemp("select")
    src, exe = d / "select_dump.cpp", d / "select_dump"
    src.write_text(HARNESS)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}", str(src), "-o", str(exe)],
                   check=True)
    token = {None: "<unset>", "": "<empty>"}
    lines = [" ".join(map(str, [api, t, W, device, kind, token.get(a, a)])) for api, t, W, device, kind, a in cases()]
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout
    rows = [tuple(map(int, l.split())) for l in out.splitlines()]
    assert len(rows) == len(lines) == 5 * 4 * 6 * 2 * 4 * 8
    return rows


def test_select_is_the_parent_rules_on_the_whole_grid(selected):
    seen = set()
    for case, (_, path, _) in zip(cases(), selected):
        assert path == parent_path(*case), case
        seen.add((case[0], path))
    reached = {ALL_REDUCE: range(7), REDUCE_SCATTER: (LOCAL, DIRECT, HOST_DIRECT, WIDE_STAGED, GROUPED, RING),
               REDUCE: (LOCAL, DIRECT, WIDE_STAGED, RING), ALL_GATHER: (LOCAL, DIRECT, RING),
               BROADCAST: (LOCAL, DIRECT, RING)}
    assert seen == {(api, p) for api, paths in reached.items() for p in paths}


def test_parse_algo(selected):
    for case, (name, _, _) in zip(cases(), selected):
        assert name == parent_name(case[5]), case[5]


def test_slots_follow_the_path(selected):
    """2^floor(log2 W) exactly when the path is Rabenseifner, W otherwise: what a packed group is laid out by."""
    for case, (_, path, slots) in zip(cases(), selected):
        W = case[2]
        assert slots == (1 << (W.bit_length() - 1) if path == RABENSEIFNER else W), case
        if path == RABENSEIFNER:  # the old predicate run_packed asked
            assert runs_rabenseifner(case[0], case[1], W, bool(case[3]), case[5]), case
        else:
            assert not runs_rabenseifner(case[0], case[1], W, bool(case[3]), case[5]) or path == WIDE_STAGED, case


def test_the_orders_that_are_easy_to_get_wrong(selected):
    got = dict(zip(cases(), (row[1] for row in selected)))
    assert got[(ALL_REDUCE, IPC, 3, 1, BUILTIN, "rabenseifner")] == DIRECT        # IPC has no other form
    assert got[(ALL_REDUCE, THREADS, 3, 1, BUILTIN, "rabenseifner")] == RABENSEIFNER
    assert got[(ALL_REDUCE, THREADS, 9, 1, BUILTIN, None)] == RING                 # above one node
    assert got[(ALL_REDUCE, RCCL, 8, 1, BUILTIN, "direct")] == RING                # "direct" on RCCL runs the ring
    assert got[(ALL_REDUCE, RCCL, 8, 1, PREMUL, "grouped")] == RING                # grouped: built-in ops only
    assert got[(ALL_REDUCE, RCCL, 8, 1, WIDE, "grouped")] == WIDE_STAGED           # its fp32 inside is grouped
    assert got[(ALL_REDUCE, THREADS, 8, 1, WIDE, None)] == DIRECT                  # wide chains run direct
    assert got[(ALL_REDUCE, THREADS, 8, 0, WIDE, None)] == HOST_DIRECT             # rejected by the validator
    assert got[(REDUCE, THREADS, 8, 0, BUILTIN, None)] == RING                     # no host-direct reduce
    assert got[(REDUCE, RCCL, 8, 1, BUILTIN, "grouped")] == RING                   # no grouped reduce
    assert got[(REDUCE_SCATTER, THREADS, 8, 1, BUILTIN, "rabenseifner")] == RING   # the name is ncclAllReduce's
    assert got[(ALL_REDUCE, THREADS, 1, 1, WIDE_SCALED, "ring")] == WIDE_STAGED    # W == 1: its 16 -> 16 bit pass
    assert got[(ALL_GATHER, THREADS, 1, 1, WIDE, None)] == LOCAL
