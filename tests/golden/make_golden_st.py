"""Golden vectors for structural triangulation, produced by the REFERENCE's own functions (build container only; the reference
tree is put on the path through tests/golden/ref_harness.py, nothing is copied):

  lib/structural/structural_triangulation.py::Pose3D_inference_torch (fp32, one person a call) on the 15-joint Panoptic tree,
  lib/structural/structural_triangulation.py::Pose3D_inference (fp64 numpy; its reshape(17, 3) allows the Human3.6M tree only).

    python tests/golden/make_golden_st.py        -> tests/golden/st.npz

Inputs are the seeded scenes of tests/golden/st_cases.py (rings of 3, 4 and 5 cameras, 4 persons a scene, 0 or 2 px of noise),
rounded to fp32 BEFORE the reference sees them; inputs, the trees' parent tables and the reference's outputs are stored:

  <scene>_{ud, conf, Pm, bone_len, truth}          scene = pan_v<V>_n<noise> | h36m_v<V>_n<noise>
  <scene>_<method>_<w|u>                           method = LS | ST1 | ST3; w = the scene's weights, u = None (the reference's
                                                   1 / V fallback; Panoptic scenes only); (4, J, 3) fp32 (pan) / fp64 (h36m)
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from mvgformer_amd.structural import H36M17_PARENT, PANOPTIC15_PARENT  # noqa: E402
from tests.golden import ref_harness  # noqa: E402
from tests.golden.st_cases import scene  # noqa: E402

METHODS = (("LS", "LS", 1), ("ST1", "ST", 1), ("ST3", "ST", 3))


def main():
    lib = os.path.join(ref_harness.REF_ROOT, "lib")
    if lib not in sys.path:
        sys.path.insert(0, lib)
    st = importlib.import_module("structural.structural_triangulation")
    out = {"pan_parent": np.array(PANOPTIC15_PARENT, np.int32), "h36m_parent": np.array(H36M17_PARENT, np.int32)}
    trees = {"pan": st.create_human_tree("cmupanoptic"), "h36m": st.create_human_tree("human36m")}
    for name, parent in (("pan", PANOPTIC15_PARENT), ("h36m", H36M17_PARENT)):
        tree = trees[name]
        assert [-1] + [tree.node_list[i]["parent"] for i in range(1, tree.size)] == list(parent)
        for V in (3, 4, 5):
            for noise in (0, 2):
                key = "%s_v%d_n%d" % (name, V, noise)
                sc = scene(1000 * V + 10 * noise + (name == "h36m"), V, parent, persons=4, noise=float(noise))
                for k, val in sc.items():
                    out["%s_%s" % (key, k)] = val
                for tag, method, steps in METHODS:
                    for wtag in (("w", "u") if name == "pan" else ("w",)):
                        res = []
                        for p in range(4):
                            ud, cf, bl, Pm = sc["ud"][p], sc["conf"][p], sc["bone_len"][p].reshape(-1, 1), sc["Pm"]
                            if name == "pan":
                                x = st.Pose3D_inference_torch(V, tree, torch.from_numpy(ud), torch.from_numpy(cf) if wtag == "w" else None,
                                                              torch.from_numpy(bl), torch.from_numpy(Pm), method, steps).numpy()
                                assert x.dtype == np.float32
                            else:
                                x = st.Pose3D_inference(V, tree, ud.astype(np.float64), cf.astype(np.float64), bl.astype(np.float64),
                                                        Pm.astype(np.float64), method, steps)
                                assert x.dtype == np.float64
                            res.append(x)
                        out["%s_%s_%s" % (key, tag, wtag)] = np.stack(res)
    path = os.path.join(HERE, "st.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
