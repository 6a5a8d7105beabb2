"""Restatement of the unit orders of the fp32 render MLP (include/nerf_mi355x_order.h) on the CPU: the
co-dead counts of a set of 32-point tiles, the matching that turns one layer's counts into its order, and the state dict of the
permuted network.  Test infrastructure; numpy and torch only."""
import numpy as np
import torch

from pack_reference import act_feat

RELU_FED = tuple(f"h{l}" for l in range(8))


def co_dead_counts(h):
    """h [tiles, 32, 256] post-ReLU activations of one layer (a ragged tile: pass its valid points, repeated) -> int32 [256, 256]:
    the number of tiles in which units i and j are both zero at every point."""
    off = (h <= 0).all(dim=1).to(torch.float64)                    # [tiles, 256]
    return (off.T @ off).round().to(torch.int32)


def match(counts):
    """counts [256, 256] -> order [256] (numpy int64), the rule of csrc/nerf_unit_order_match.h: pairs i < j sorted by (count
    descending, i, j ascending), taken greedily while both units are free; the 128 pairs sorted by (count descending, lower unit
    ascending) go to k-steps 0..127, the lower unit to position act_feat(t, r, 0), the higher to act_feat(t, r, 1)."""
    c = np.asarray(counts).astype(np.int64)
    i, j = np.triu_indices(256, k=1)                               # row-major: (i, j) ascending
    walk = np.lexsort((j, i, -c[i, j]))                            # last key first
    free = np.ones(256, bool)
    pairs = []
    for p in walk:
        a, b = int(i[p]), int(j[p])
        if free[a] and free[b]:
            free[a] = free[b] = False
            pairs.append((-int(c[a, b]), a, b))
            if len(pairs) == 128:
                break
    pairs.sort()
    order = np.full(256, -1, np.int64)
    for s, (_, a, b) in enumerate(pairs):
        order[act_feat(s >> 4, s & 15, 0)] = a
        order[act_feat(s >> 4, s & 15, 1)] = b
    return order


def dead_fraction(h, order=None):
    """Share of (tile, k-step) pairs the kernel skips when the layer's units sit in `order` (None: parameter order)."""
    off = (h <= 0).all(dim=1)
    if order is not None:
        off = off[:, torch.as_tensor(np.asarray(order), dtype=torch.long)]
    lo = torch.tensor([act_feat(s >> 4, s & 15, 0) for s in range(128)])
    hi = torch.tensor([act_feat(s >> 4, s & 15, 1) for s in range(128)])
    return (off[:, lo] & off[:, hi]).float().mean().item()


def random_orders(seed):
    """[8, 256] int64: eight seeded permutations."""
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(256, generator=g) for _ in range(8)])


def permute_sub_model(sub, order):
    """The 24 tensors (keys without prefix) of the same network with its hidden units permuted: unit order[l][p] of h_l sits at
    position p.  Rows of pts_linears.l and its bias; the columns of whatever reads h_l: pts_linears.(l+1) (behind the 63 skip columns
    for l = 4), and for l = 7 feature_linear and alpha_linear.  Nothing else moves."""
    order = torch.as_tensor(np.asarray(order), dtype=torch.long)
    out = {k: v.clone() for k, v in sub.items()}
    for l in range(8):
        w, b = out[f"pts_linears.{l}.weight"][order[l]], out[f"pts_linears.{l}.bias"][order[l]]
        if l > 0:
            skip = 63 if l == 5 else 0
            w = torch.cat([w[:, :skip], w[:, skip:][:, order[l - 1]]], dim=1)
        out[f"pts_linears.{l}.weight"], out[f"pts_linears.{l}.bias"] = w.contiguous(), b.contiguous()
    for name in ("feature_linear.weight", "alpha_linear.weight"):
        out[name] = out[name][:, order[7]].contiguous()
    return out


def permute_state_dict(sd, orders):
    """sd with "model." / "model_fine." prefixes, orders {"model": [8,256], "model_fine": [8,256]} (a missing prefix stays)."""
    out = {k: v.clone() for k, v in sd.items()}
    for prefix, order in orders.items():
        sub = {k[len(prefix) + 1:]: v for k, v in sd.items() if k.startswith(prefix + ".")}
        for k, v in permute_sub_model(sub, order).items():
            out[f"{prefix}.{k}"] = v
    return out
