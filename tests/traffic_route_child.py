"""The fresh process of test_gpu_traffic_route.py's .npz test: build the loop with route vehicles again (its specs carry their own
route arrays, so the new engine's table is registered from them), take the checkpoints of the file, go on from slot `slot` for
`ticks` ticks, and write what the recorder then holds of those ticks.
    python tests/traffic_route_child.py <checkpoints.npz> <slot> <ticks> <out.npz>"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import traffic_route_cases as RC  # noqa: E402


def main(path, slot, ticks, out):
    pkg = RC.package()
    loop = RC.scenario_loop(pkg, RC.routes_of(pkg), checkpoint_every=RC.EVERY)
    assert loop.checkpoints == [] and len(loop.loop.eng.traffic_routes) == 3
    loop.load_checkpoints(path)
    loop.restore(slot)
    k0 = dict(loop.checkpoints)[slot]
    loop.run(ticks)
    rec = loop.recorder
    np.savez(out, k0=k0, rec=rec.rec[k0:k0 + ticks].cpu().numpy(), flags=rec.flags[k0:k0 + ticks].cpu().numpy(),
             obs=rec.obs[k0:k0 + ticks].cpu().numpy(), ticks_run=rec.ticks_run, x0=loop.loop.x0.cpu().numpy(),
             obs_state=loop.obst.state.cpu().numpy())


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
