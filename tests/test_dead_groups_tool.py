"""tools/dead_ksteps.py, the dead-group columns (CPU): all-dead 4-k-step groups per tile, the leading run the kernel steps over
(csrc/nerf_mlp_f32.hip.inc, gemm_tiles `prefix`) and the number of runs, on a hand-made activation tensor."""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import dead_ksteps as dk  # noqa: E402


def _tile(dead_groups, point=7):
    """[32, 256] activations whose k-steps are dead exactly in the given groups: every other k-step has one of its two features
    positive at one point."""
    h = torch.zeros(32, 256)
    pairs = dk.kstep_pairs()
    for s in range(128):
        if s // 4 not in dead_groups:
            h[point, pairs[s][s & 1]] = 1.0 + s
    return h


# (dead groups, all-dead, leading run, runs)
TILES = (
    (set(range(5)) | {10, 11, 12}, 8, 5, 2),          # a prefix of five and one interior run
    (set(range(32)), 32, 32, 1),                      # a wholly dead input
    ({31}, 1, 0, 1),                                  # no prefix: the only dead group is the last
    (set(), 0, 0, 0),
    ({0, 2, 4, 6}, 4, 1, 4),                          # a prefix of one, three more runs of one
    (set(range(1, 32)), 31, 0, 1),                    # group 0 alive: everything behind it is outside the prefix
)


def _acts():
    return torch.stack([_tile(g, point=3 * i) for i, (g, *_) in enumerate(TILES)])


def test_dead_groups_of_known_tiles():
    dead = dk.dead_ksteps(_acts())
    for i, (groups, *_rest) in enumerate(TILES):
        assert dead[i].reshape(32, 4).all(-1).nonzero().flatten().tolist() == sorted(groups)
    n, lead, runs = dk.dead_groups(dead)
    assert n.tolist() == [t[1] for t in TILES]
    assert lead.tolist() == [t[2] for t in TILES]
    assert runs.tolist() == [t[3] for t in TILES]
    assert dk.stepped_over(lead).tolist() == [min(t[2], 31) for t in TILES]      # the kernel never steps over the last group


def test_a_group_with_one_live_row_is_not_dead():
    h = _tile(set(range(8)))
    h[31, dk.kstep_pairs()[4 * 3 + 3][1]] = 0.5          # the last row of group 3, at the last point only
    n, lead, runs = dk.dead_groups(dk.dead_ksteps(h[None]))
    assert (n.item(), lead.item(), runs.item()) == (7, 3, 2)


def test_count_reports_the_columns_per_gemm_and_order():
    acts = {f"h{l}": _acts() for l in range(8)}
    raw = torch.ones(len(TILES), 32, 4)
    plain = dk.count(raw, acts, density_only=False, skip_dead_colour=False)
    mean = lambda k: sum(t[k] for t in TILES) / len(TILES)
    fed = [r for r in plain["rows"] if r["kstep_dead"] is not None]
    assert len(fed) == 8
    for row in fed:
        assert abs(row["groups_dead"] - mean(1)) < 1e-6 and abs(row["groups_leading"] - mean(2)) < 1e-6
        assert abs(row["group_runs"] - mean(3)) < 1e-6 and "groups_dead_repaired" not in row
        stepped = 0.0 if row["gemm"].startswith("views") else sum(min(t[2], 31) for t in TILES) / len(TILES)
        assert abs(row["groups_stepped"] - stepped) < 1e-6                    # (the views GEMM has no group path)
    assert all("groups_dead" not in r for r in plain["rows"] if r["kstep_dead"] is None)
    # the identity order reports the plain figures again
    ident = {f"h{l}": list(range(256)) for l in range(8)}
    same = dk.count(raw, acts, False, False, orders=ident)
    for a, b in zip(fed, [r for r in same["rows"] if r["kstep_dead"] is not None]):
        assert (b["groups_dead_repaired"], b["groups_leading_repaired"], b["group_runs_repaired"]) == (a["groups_dead"], a["groups_leading"], a["group_runs"])
    # an order that mirrors the 32 groups (the units of group g go to group 31 - g, row by row): trailing runs become leading ones
    pairs = dk.kstep_pairs()
    rev = torch.empty(256, dtype=torch.long)
    for s in range(128):
        m = (31 - s // 4) * 4 + (s & 3)
        rev[pairs[s][0]], rev[pairs[s][1]] = pairs[m][0], pairs[m][1]
    moved = dk.count(raw, acts, False, False, orders={f"h{l}": rev.tolist() for l in range(8)})
    want_lead = [0, 32, 1, 0, 0, 31]                      # the mirrored tiles: trailing runs become leading ones
    row = [r for r in moved["rows"] if r["kstep_dead"] is not None][0]
    assert abs(row["groups_leading_repaired"] - sum(want_lead) / len(TILES)) < 1e-6
    assert abs(row["groups_dead_repaired"] - mean(1)) < 1e-6 and abs(row["group_runs_repaired"] - mean(3)) < 1e-6
