"""Probe of the fused Kin loop's FK-walk cache (cdx_kin_opt_buffers::fk_state) after a short loop: are the q-check
slots the final joint rows (so the next iteration's check passes), and is the cached final pose the walk's?

  python tools/fk_cache_probe.py
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from compliancedex_amd import KinGraspOptimizer
    from compliancedex_amd.workloads import banana_mesh, config4_kin_inputs
    E = 256
    links, offs, palm, q, target, comp = config4_kin_inputs(E, device="cuda", q_scale=0.05)
    kin = KinGraspOptimizer("iiwa7_allegro", links, offs, palm_offset=palm.tolist(), num_iters=3, optimize_target=True,
                            ref_q=[0.0] * 23)
    args = [torch.from_numpy(a).to("cuda") for a in (q, target, comp)]
    kin.optimize(*args, 1, banana_mesh(), verbose=False, trace_rows=True)
    torch.cuda.synchronize()
    st = kin.last_loop
    from compliancedex_amd.optimizers import kin_fk_cache_qcheck, kin_fk_cache_view
    view = kin_fk_cache_view(st.fk_state, 13)  # iiwa7_allegro's deepest fingertip path: the 16-level layout
    same = view["qcheck"][:4 * E] == kin_fk_cache_qcheck(st.pose.view(E, -1))
    ok, bad = int(same.sum()), int((~same).sum())
    tags = view["tag"][:4 * E].tolist()
    R0 = view["pose"][0, :9]
    print(json.dumps({"qcheck_ok": ok, "qcheck_bad": bad, "tags": sorted(set(tags)), "iterations": 3,
                      "R_lane0": R0.tolist()}))


if __name__ == "__main__":
    main()
