"""One-to-one matcher fixtures produced by RUNNING THE REFERENCE's own matcher on the CPU.

Build container only (needs the reference tree and scipy; nothing is copied):

    python -m tests.golden.make_golden_hungarian

What runs, unmodified and loaded by path: ``HungarianMatcher`` of lib/models/matcher.py with methods 'hungarian' / 'hungarian-dis'
-- its fp32 cost matrix and ``scipy.optimize.linear_sum_assignment`` per batch element -- on the inputs of
tests/hungarian_cases.py (GOLDEN), once per set of predictions (Lm), with ``meta[0]['joints_3d_norm']`` made in fp32 as
dq_transformer.py:499-500 makes it and grid_size / grid_center set as SetCriterion sets them.  Stored per case: a checksum of the
inputs and, per (l, b), the reference's (query, person) pairs.  The maker prints, and asserts to be far above fp32 rounding, the gap
between the optimum and the best assignment that differs from it in one person's query.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import hungarian_cases as HC  # noqa: E402
from tests import hungarian_ref as H  # noqa: E402
from tests.golden.ref_harness import REF_ROOT  # noqa: E402


def load_matcher_module():
    spec = importlib.util.spec_from_file_location("reference_matcher", os.path.join(REF_ROOT, "lib", "models", "matcher.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def swap_gap(C, q, g):
    """smallest increase of the total cost when one person moves to a free query (a lower bound on nothing, an indicator of how far
    the optimum is from its nearest neighbours)"""
    free = np.ones(C.shape[1], bool)
    free[q] = False
    if not free.any():
        return np.inf
    return float(min(C[gi, free].min() - C[gi, qi] for qi, gi in zip(q, g)))


def main():
    mod = load_matcher_module()
    out = {}
    size = torch.tensor(HC.SPACE_SIZE)
    cen = torch.tensor(HC.SPACE_CENTER)
    for name in HC.GOLDEN:
        c = HC.CASES[name]
        inp = HC.make_inputs(name)
        matcher = mod.HungarianMatcher("abs", "norm", cost_class=c["cost_class"], cost_pose=c["cost_pose"], method=c["method"])
        matcher.grid_size, matcher.grid_center = size, cen
        gt = torch.from_numpy(inp["joints_3d"])
        meta = [dict(joints_3d=gt, joints_3d_norm=(gt - cen + size / 2.0) / size, num_person=torch.from_numpy(inp["num_person"]))]
        restated = H.hungarian_match(inp["poses"], inp["joints_3d"], inp["num_person"], HC.SPACE_SIZE, HC.SPACE_CENTER,
                                     logits=inp["logits"], **HC.match_kwargs(name))
        gap = np.inf
        for l in range(c["Lm"]):
            outputs = {"pred_logits": torch.from_numpy(inp["logits"][l]), "pred_poses": {"outputs_coord": torch.from_numpy(inp["poses"][l])}}
            for b, (q, g) in enumerate(matcher(outputs, meta)):
                out["%s/%d/%d/query" % (name, l, b)] = q.numpy().astype(np.int32)
                out["%s/%d/%d/gt" % (name, l, b)] = g.numpy().astype(np.int32)
                gap = min(gap, swap_gap(restated["C"][l, b, :len(q)], q.numpy(), g.numpy()))
        out[name + "/checksum"] = HC.checksum(inp)
        print("%-10s single-move gap %.4g" % (name, gap))
        assert gap > 1e-3 or not np.isfinite(gap), (name, gap)      # costs ~1e1..1e3: fp32 rounding ~1e-4 at most
    path = os.path.join(HERE, "hungarian.npz")
    np.savez_compressed(path, **out)
    print("hungarian.npz %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
