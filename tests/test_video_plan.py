"""kbe_render_video's launch plan (ken-burns-effect_amd/csrc/kbe_video_plan.h: plain C++ on indices) on the host: the C++ checker
next to this file sweeps the invariants and prints single plans for the worked cases."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, os.pardir, 'ken-burns-effect_amd', 'csrc')
HBM, PER_FRAME, GROUPS, RING = range(4)
FAST_RAMP, EVEN_GROUPS, FUSED, AHEAD = 1, 2, 4, 8


@pytest.fixture(scope='module')
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('video_plan') / 'video_plan_check')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-I', CSRC, os.path.join(HERE, 'video_plan_check.cpp'), '-o', exe])
    return exe


def plan(checker, dest, n, lanes, group, batch, flags=0):
    """[(unit lane, first, count, [(launch lane, [frame, ...]), ...]), ...]"""
    out = subprocess.run([checker, str(dest), str(n), str(lanes), str(group), str(batch), str(flags)], capture_output=True, text=True, check=True)
    units = []
    for line in out.stdout.splitlines():
        words = line.split()
        if words[0] == 'unit':
            units.append((int(words[1]), int(words[2]), int(words[3]), []))
        else:
            units[-1][3].append((int(words[1]), [int(f.split(':')[0]) for f in words[4:]]))
    return units


def test_video_plan_invariants(checker):
    """n_frames 0..140, lanes 1..8, frames per launch 1..12, every destination, ramp and route: every frame once, launches of at most
    `group` frames, transfer groups consecutive on the ramp of include/kbe.h and on lane g % lanes, every bucket scratch set splats into
    clear z-buffers and ends with A clear, placements ahead only into the same lane's next launch and never into a larger one."""
    out = subprocess.run([checker], capture_output=True, text=True)
    plans, failures = (int(v) for v in out.stdout.split())
    assert out.returncode == 0 and failures == 0 and plans > 1_000_000, out.stderr


@pytest.mark.parametrize('flags, starts', [(0, [0, 1, 3, 7, 15]), (FAST_RAMP, [0, 1, 4, 11]), (EVEN_GROUPS, [0, 16])])
def test_video_plan_transfer_group_ramp(checker, flags, starts):
    units = plan(checker, GROUPS, 20, 2, 16, -16, flags)
    assert [u[1] for u in units] == starts
    assert [u[2] for u in units] == [b - a for a, b in zip(starts, starts[1:] + [20])]
    assert [u[0] for u in units] == [g % 2 for g in range(len(starts))]


def test_video_plan_hbm_chunks_are_consecutive_frames(checker):
    units = plan(checker, HBM, 10, 4, 2, 0, FUSED | AHEAD)
    assert [launch for u in units for launch in u[3]] == [(0, [0, 1]), (1, [2, 3]), (2, [4, 5]), (3, [6, 7]), (0, [8, 9])]
