"""The block -> tile maps of the combine kernels (dccl_amd/csrc/tile_maps.hpp), on the CPU: the header has no
HIP include, so g++ compiles it into a harness that checks every map exhaustively and prints one verdict per
section.  Every kernel's coverage of its tiles rests on these maps being bijections on [0, grid) (kOrderXcd on a
grid that is a multiple of 8), on tile_order (runtime order) and first_tile (template order) being the same map,
and on the strided walk `t = first(b); t < ntiles; t += grid` visiting every tile once at the launchers' own grids
and at the capped grids a grid_cap can produce.  The test-only clamp DCCL_MAX_GRID_TEST (max_grid(), where launch()
clamps every grid) is parsed here, the walks are repeated under it at 8 and 104, and the plan of
tests/test_gpu_grid_stride_small.py, which runs the kernels under those clamps, is checked without a GPU."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dccl_amd", "csrc")

HARNESS = r"""
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "tile_maps.hpp"
using namespace dccl_amd;

typedef size_t (*Map)(size_t, size_t);
template <int O> size_t order_rt(size_t b, size_t g) { return tile_order(O, b, g); }
template <int O> size_t order_ct(size_t b, size_t g) { return first_tile<O>(b, g); }
// maps any grid may take (the vector, shifted and phased kernels) ...
static const Map kAnyGrid[] = {xcd_remap, run_tile<1>, run_tile<2>, run_tile<4>, run_tile<8>};
static const char* kAnyGridName[] = {"xcd_remap", "run_tile<1>", "run_tile<2>", "run_tile<4>", "run_tile<8>"};
static const int kRuns[] = {1, 2, 4, 8};
// ... and the orders of the misaligned-destination kernels (grids that are multiples of 8)
static const Map kOrderRt[] = {order_rt<0>, order_rt<1>, order_rt<2>, order_rt<3>, order_rt<4>};
static const Map kOrderCt[] = {order_ct<0>, order_ct<1>, order_ct<2>, order_ct<3>, order_ct<4>};

static std::vector<unsigned char> seen(kMaxGrid);

struct Section {
    const char* name;
    long n = 0;
    std::string fail;
    void bad(const char* what, const char* map, size_t a, size_t b, size_t c) {
        if (!fail.empty()) return;
        char buf[256];
        std::snprintf(buf, sizeof buf, "%s %s (%zu, %zu, %zu)", what, map, a, b, c);
        fail = buf;
    }
    void print(bool last = false) const {
        std::printf("\"%s\": {\"ok\": %s, \"n\": %ld, \"fail\": \"%s\"}%s", name, fail.empty() ? "true" : "false", n,
                    fail.c_str(), last ? "" : ", ");
    }
};

// every value in [0, g), none twice
static bool bijective(Map f, size_t g) {
    std::memset(seen.data(), 0, g);
    for (size_t b = 0; b < g; ++b) {
        const size_t t = f(b, g);
        if (t >= g || seen[t]) return false;
        seen[t] = 1;
    }
    return true;
}

// the kernels' walk: every tile in [0, ntiles) exactly once, none outside
static bool covers(Map f, size_t g, size_t ntiles) {
    std::memset(seen.data(), 0, ntiles + 1);
    size_t visits = 0;
    for (size_t b = 0; b < g; ++b)
        for (size_t t = f(b, g); t < ntiles; t += g) {
            if (seen[t]) return false;
            seen[t] = 1;
            ++visits;
        }
    return visits == ntiles;
}

// With an argument: the parse of DCCL_MAX_GRID_TEST and the walks at min(the launcher's grid, max_grid()), which
// is what launch() hands the kernels in a process that carries the variable.
static int clamped_main() {
    Section parse{"parse"};
    const struct { const char* text; size_t want; } cases[] = {
        {"8", 8}, {"104", 104}, {"16777216", kMaxGrid},
        {nullptr, kMaxGrid}, {"", kMaxGrid}, {"104x", kMaxGrid}, {"8 ", kMaxGrid}, {" 8", kMaxGrid}, {"+8", kMaxGrid},
        {"-8", kMaxGrid}, {"0x10", kMaxGrid}, {"0", kMaxGrid}, {"4", kMaxGrid}, {"12", kMaxGrid}, {"100", kMaxGrid},
        {"16777224", kMaxGrid}, {"99999999999999999999999", kMaxGrid}};
    for (const auto& c : cases) {
        const size_t got = parse_max_grid(c.text);
        if (got != c.want) parse.bad("parse", c.text ? c.text : "(null)", got, c.want, 0);
        ++parse.n;
    }
    const size_t mg = max_grid();
    Section cov{"clamped_coverage"}, part{"clamped_partial_owner"};
    for (size_t ntiles = 0; ntiles <= 700; ++ntiles) {
        const size_t own_any = ntiles ? ntiles : 1, own_8 = unaligned_grid(ntiles * 64);
        const size_t g_any = own_any < mg ? own_any : mg, g_8 = own_8 < mg ? own_8 : mg;
        for (int m = 0; m < 5; ++m) {
            if (!covers(kAnyGrid[m], g_any, ntiles)) cov.bad("coverage", kAnyGridName[m], ntiles, g_any, 0);
            ++cov.n;
        }
        for (int o = 0; o < 5; ++o) {
            if (!covers(kOrderRt[o], g_8, ntiles)) cov.bad("coverage", "tile_order", size_t(o), ntiles, g_8);
            if (!covers(kOrderCt[o], g_8, ntiles)) cov.bad("coverage", "first_tile", size_t(o), ntiles, g_8);
            cov.n += 2;
        }
        const size_t nfull = ntiles, own = nfull + 1, g = own < mg ? own : mg;  // reduce_vec_kernel's partial tile
        for (int m = 0; m < 5; ++m) {
            int owners = 0;
            for (size_t b = 0; b < g; ++b) owners += kAnyGrid[m](b, g) == nfull % g;
            if (owners != 1) part.bad("owners of the partial tile", kAnyGridName[m], nfull, g, size_t(owners));
            if (!covers(kAnyGrid[m], g, nfull)) part.bad("full tiles", kAnyGridName[m], nfull, g, 0);
            ++part.n;
        }
    }
    std::printf("{\"max_grid\": %zu, ", mg);
    parse.print(); cov.print(); part.print(true);
    std::printf("}\n");
    return 0;
}

int main(int argc, char**) {
    if (argc > 1) return clamped_main();
    std::vector<size_t> grids;
    for (size_t g = 1; g <= 2048; ++g) grids.push_back(g);
    grids.push_back(kMaxGrid);

    Section bij{"bijections"};
    for (size_t g : grids)
        for (int m = 0; m < 5; ++m) {
            if (!bijective(kAnyGrid[m], g)) bij.bad("not a bijection", kAnyGridName[m], g, 0, 0);
            ++bij.n;
        }

    // run_tile<R>: block 8 R q + r of a full group takes tile 8 R q + R (r % 8) + r / 8; a partial last group
    // keeps the identity
    Section form{"run_formula"};
    for (size_t g : grids)
        for (int i = 0; i < 4; ++i) {
            const size_t R = size_t(kRuns[i]), span = 8 * R;
            const Map f = kAnyGrid[1 + i];
            for (size_t b = 0; b < g; ++b) {
                const size_t q = b / span, r = b % span;
                const bool full_group = (q + 1) * span <= g;
                const size_t want = full_group ? span * q + R * (r % 8) + r / 8 : b;
                if (f(b, g) != want) form.bad(full_group ? "full group" : "partial group", kAnyGridName[1 + i], b, g, f(b, g));
            }
            ++form.n;
        }

    Section ord{"orders"};
    for (int o = 0; o < 5; ++o)
        for (size_t g = 8; g <= 2048; g += 8) {
            if (!bijective(kOrderRt[o], g)) ord.bad("not a bijection", "tile_order", size_t(o), g, 0);
            for (size_t b = 0; b < g; ++b)
                if (kOrderRt[o](b, g) != kOrderCt[o](b, g)) ord.bad("tile_order != first_tile", "order", size_t(o), b, g);
            ++ord.n;
        }
    for (int o = 0; o < 5; ++o) {  // and at the largest grid
        if (!bijective(kOrderRt[o], kMaxGrid)) ord.bad("not a bijection", "tile_order", size_t(o), kMaxGrid, 0);
        for (size_t b = 0; b < kMaxGrid; ++b)
            if (kOrderRt[o](b, kMaxGrid) != kOrderCt[o](b, kMaxGrid)) ord.bad("tile_order != first_tile", "order", size_t(o), b, kMaxGrid);
        ++ord.n;
    }

    Section grid{"grids"};
    if (kMaxGrid % 8 != 0) grid.bad("kMaxGrid % 8", "kMaxGrid", kMaxGrid, 0, 0);
    for (size_t nvec = 0; nvec <= 64 * 2100; ++nvec) {
        const size_t g = unaligned_grid(nvec), ntiles = (nvec + 63) / 64;
        // a multiple of 8, at least 8, one block per tile, and the smallest such
        if (g % 8 != 0 || g < 8 || g < ntiles || (g > 8 && g >= ntiles + 8)) grid.bad("grid", "unaligned_grid", nvec, g, ntiles);
        ++grid.n;
    }
    for (size_t nvec : {size_t(1) << 26, (size_t(1) << 30) + 1, (size_t(1) << 40) - 1}) {
        const size_t g = unaligned_grid(nvec);
        if (g % 8 != 0 || g < (nvec + 63) / 64) grid.bad("grid", "unaligned_grid", nvec, g, 0);
        ++grid.n;
    }

    // the strided walk at the launcher's own grid, at the capped grids 8, 16, 64 (grid_cap / 8 * 8), and at
    // min(own, cap), which is what a capped launch really gets
    Section cov{"coverage"};
    const size_t caps[] = {8, 16, 64};
    for (size_t ntiles = 0; ntiles <= 700; ++ntiles) {
        const size_t own_any = ntiles ? ntiles : 1;              // ceil_div(nvec, TILE), 1 for edge scalars alone
        const size_t own_8 = unaligned_grid(ntiles * 64);        // the misaligned-destination launchers
        std::vector<size_t> g_any = {own_any}, g_8 = {own_8};
        for (size_t c : caps) {
            g_any.push_back(c);
            g_any.push_back(own_any < c ? own_any : c);
            g_8.push_back(c);
            g_8.push_back(own_8 < c ? own_8 : c);
        }
        for (int m = 0; m < 5; ++m)
            for (size_t g : g_any) {
                if (!covers(kAnyGrid[m], g, ntiles)) cov.bad("coverage", kAnyGridName[m], ntiles, g, 0);
                ++cov.n;
            }
        for (int o = 0; o < 5; ++o)
            for (size_t g : g_8) {
                if (!covers(kOrderRt[o], g, ntiles)) cov.bad("coverage", "tile_order", size_t(o), ntiles, g);
                if (!covers(kOrderCt[o], g, ntiles)) cov.bad("coverage", "first_tile", size_t(o), ntiles, g);
                cov.n += 2;
            }
    }

    // reduce_vec_kernel: full tiles by the walk, the partial last tile to the block with bid == nfull % grid:
    // exactly one block
    Section part{"vec_partial_owner"};
    for (size_t nfull = 0; nfull <= 700; ++nfull) {
        const size_t own = nfull + 1;  // ceil_div(nvec, TILE) with a partial tile
        for (size_t g : {own, size_t(8), size_t(16), size_t(64), own < 8 ? own : size_t(8), own < 64 ? own : size_t(64)})
            for (int m = 0; m < 5; ++m) {
                int owners = 0;
                for (size_t b = 0; b < g; ++b) owners += kAnyGrid[m](b, g) == nfull % g;
                if (owners != 1) part.bad("owners of the partial tile", kAnyGridName[m], nfull, g, size_t(owners));
                if (!covers(kAnyGrid[m], g, nfull)) part.bad("full tiles", kAnyGridName[m], nfull, g, 0);
                ++part.n;
            }
    }

    std::printf("{");
    bij.print(); form.print(); ord.print(); grid.print(); cov.print(); part.print(true);
    std::printf("}\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("tile_maps")
    src, exe = d / "tile_maps_check.cpp", d / "tile_maps_check"
    src.write_text(HARNESS)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{CSRC}", str(src), "-o", str(exe)],
                   check=True)
    return str(exe)


@pytest.fixture(scope="module")
def verdict(harness):
    env = {k: v for k, v in os.environ.items() if k != "DCCL_MAX_GRID_TEST"}
    return json.loads(subprocess.run([harness], check=True, capture_output=True, text=True, timeout=300,
                                     env=env).stdout)


def clamped_verdict(harness, value):
    """The harness's clamped sections in a process whose DCCL_MAX_GRID_TEST is `value` (None: unset)."""
    env = {k: v for k, v in os.environ.items() if k != "DCCL_MAX_GRID_TEST"}
    if value is not None:
        env["DCCL_MAX_GRID_TEST"] = value
    return json.loads(subprocess.run([harness, "clamped"], check=True, capture_output=True, text=True, timeout=300,
                                     env=env).stdout)


def _passed(verdict, section, n):
    v = verdict[section]
    assert v["ok"], v["fail"]
    assert v["n"] == n, (section, v["n"])  # no loop ran empty


def test_header_has_no_hip_include():
    text = open(os.path.join(CSRC, "tile_maps.hpp")).read()
    assert "#include <hip" not in text and "hip_runtime" not in text


def test_remap_and_runs_are_bijections(verdict):
    """xcd_remap(., g) and run_tile<1|2|4|8>(., g) on [0, g) for every g in 1..2048 and g = kMaxGrid."""
    _passed(verdict, "bijections", 5 * 2049)


def test_run_tile_formula_and_partial_group(verdict):
    """Inside a full group of 8 R blocks, block 8 R q + r takes tile 8 R q + R (r % 8) + r / 8; a partial last
    group keeps the identity: every block of every g in 1..2048 and of kMaxGrid, R = 1, 2, 4, 8."""
    _passed(verdict, "run_formula", 4 * 2049)


def test_tile_order_is_a_bijection_and_equals_first_tile(verdict):
    """Every order value, every grid that is a multiple of 8 in 8..2048 and kMaxGrid."""
    _passed(verdict, "orders", 5 * 256 + 5)


def test_grids_are_multiples_of_8(verdict):
    _passed(verdict, "grids", 64 * 2100 + 1 + 3)


def test_strided_walk_visits_every_tile_once(verdict):
    """t = first(b); t < ntiles; t += g over all b, for ntiles in 0..700, every map, g = the launcher's own grid,
    8, 16, 64 and min(own, cap)."""
    _passed(verdict, "coverage", 701 * (5 * 7 + 5 * 7 * 2))


def test_vec_kernel_partial_tile_has_one_owner(verdict):
    """reduce_vec_kernel hands the partial last tile to the block with bid == nfull % grid: exactly one."""
    _passed(verdict, "vec_partial_owner", 701 * 6 * 5)


KMAXGRID = 1 << 24


def test_max_grid_parse(harness):
    """parse_max_grid accepts 8, 104 and 2^24 and turns everything else into kMaxGrid (null, empty, trailing
    characters, a sign, a space, 0, 4, 12, 100, kMaxGrid + 8, an overflow); max_grid() reads the environment."""
    _passed(clamped_verdict(harness, None), "parse", 17)
    for value, want in ((None, KMAXGRID), ("", KMAXGRID), ("8", 8), ("104", 104), (str(KMAXGRID), KMAXGRID),
                        ("104x", KMAXGRID), ("0", KMAXGRID), ("4", KMAXGRID), ("12", KMAXGRID), ("100", KMAXGRID),
                        (str(KMAXGRID + 8), KMAXGRID)):
        assert clamped_verdict(harness, value)["max_grid"] == want, value


@pytest.mark.parametrize("value", [None, "8", "104"])
def test_strided_walk_under_the_test_clamp(harness, value):
    """The walks of test_strided_walk_visits_every_tile_once and test_vec_kernel_partial_tile_has_one_owner at
    min(the launcher's own grid, max_grid()) for ntiles in 0..700: up to 88 passes at 8, up to 7 at 104."""
    v = clamped_verdict(harness, value)
    assert v["max_grid"] == (KMAXGRID if value is None else int(value))
    _passed(v, "clamped_coverage", 701 * (5 + 5 * 2))
    _passed(v, "clamped_partial_owner", 701 * 5)


def test_grid_stride_plan_is_the_stated_product():
    """tests/test_gpu_grid_stride_small.py without a GPU: every family's plan has the stated number of cases, every
    planned case at least 2 * 104 + 1 tiles by its count, dtype and destination offset."""
    from tests import test_gpu_grid_stride_small as stride
    stride.check_plan()
