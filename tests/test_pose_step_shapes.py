"""Every shape of tests/pose_step_shapes.py selects the kernel forms it is there for.  No GPU: a stand-alone program prints the
plans of csrc/pose_plan.h for the rows, asked for as genpc_pose_loss_grad_batch asks, under the address and undefined-behaviour
sanitizers.  A threshold moved in the header fails here; tests/test_gpu_pose_step_batch.py would otherwise quietly stop covering
a form."""
import os
import shutil
import subprocess

import pytest

import pose_step_shapes as shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genpc_amd", "csrc")
FIELDS = "b nc np elements ride g_t g_g gb sub8 fuse_w gp gs lin_nc lin_nc_np lin_8nc".split()


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("pose_step_shapes") / "pose_step_shapes_plan")
    # (the sanitizers' runtimes linked statically, as tests/test_pose_plan.py does for its program)
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", CSRC, os.path.join(ROOT, "tests", "pose_step_shapes_plan.cpp"), "-o", exe], check=True)
    args = []
    for r in shapes.ROWS:
        args += [str(r.b), str(r.nc), str(r.np), repr(r.radius), str(r.size), str(int(r.mask))]
    out = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert out.returncode == 0, out.stdout
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(shapes.ROWS), out.stdout
    return {r.id: dict(zip(FIELDS, map(int, line.split()))) for r, line in zip(shapes.ROWS, lines)}


def test_the_table_is_the_issue_s():
    assert [r.id for r in shapes.ROWS] == ["A", "B", "C", "D", "Dcd", "E", "Ecd", "F", "G"]
    assert len(shapes.BY_ID) == len(shapes.ROWS) and len(shapes.FULL) == 7 and len(shapes.CD_ONLY) == 2
    assert all(r.must for r in shapes.ROWS)


@pytest.mark.parametrize("row", shapes.ROWS, ids=lambda r: r.id)
def test_row_selects_its_forms(plans, row):
    p = plans[row.id]
    assert (p["b"], p["nc"], p["np"], p["elements"]) == (row.b, row.nc, row.np, row.b), p
    # one stream: with the full objective pose_grad's blocks always ride, without it there is nothing to ride in
    assert p["ride"] == int(row.mask), p
    got = dict(p)
    got["b_mod_8"] = int(p["elements"] % 8 != 0)          # (the elements the plan launches: which mapping xcd_block takes)
    got["lin_nc_even"] = int(p["lin_nc"] % 2 == 0)
    got["lin_8nc_even"] = int(p["lin_8nc"] % 2 == 0)
    for name, want in row.must.items():
        assert got[name] == want, (row.id, name, got[name], want, p)
    if row.id in ("D", "Dcd"):          # the cap bites: a block of pose_grad walks its points in more than one pass
        assert p["g_g"] < p["lin_nc_np"], p
    if row.id in ("F", "G"):            # 8 / 4 = two XCDs per image needs an even grid per image (mask.h xcd_block, second mapping)
        assert row.b == 4


def test_thresholds_sit_where_the_rows_assume(plans):
    """A and B are one point apart across the lanes-per-point threshold; B and C differ in the radius alone."""
    A, B, C = shapes.BY_ID["A"], shapes.BY_ID["B"], shapes.BY_ID["C"]
    assert (B.b, B.nc - 1, B.np, B.radius, B.size) == (A.b, A.nc, A.np, A.radius, A.size)
    assert plans["A"]["sub8"] == 1 and plans["B"]["sub8"] == 0
    assert (C.b, C.nc, C.np, C.size) == (B.b, B.nc, B.np, B.size) and C.radius != B.radius
    assert plans["B"]["fuse_w"] == 0 and plans["C"]["fuse_w"] == 1


def test_the_chosen_draws_keep_the_rules(oracle):
    """tests/pose_step_shapes.py RESEED against the procedure that made it (tests/pose_step_select.py), on the CPU oracle: every
    chosen draw keeps rule (a), total losses of a row pairwise three tolerances apart in every renderer and colouring, and rule
    (b), the oracle's own gradient within a quarter tolerance under one-ulp moves of parameters and centre.  If _shape or
    _colours of test_gpu_geometry.py change, or the oracle does, this fails and the table is to be made again
    (python tests/pose_step_select.py)."""
    import pose_step_select as sel
    seeds = {r.seed: r for r in shapes.FULL}
    assert set(shapes.RESEED) <= set(seeds)
    for seed, draws in shapes.RESEED.items():
        assert all(0 <= e < seeds[seed].b and 0 < k < sel.kMaxDraws for e, k in draws.items()), (seed, draws)
    for row in shapes.ROWS:
        prev = []
        for e in range(row.b):
            x = shapes.element(row, e)
            cur = sel.evaluate(oracle, row, x)
            assert all(sel.apart(row, cur, p) for p in prev), (row.id, e)
            c = sel.conditioning(oracle, row, e, x, cur)
            assert c < sel.kCond, (row.id, e, c)
            prev.append(cur)
