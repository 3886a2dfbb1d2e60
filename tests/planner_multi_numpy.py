"""Numpy restatement of the multi-trajectory planner's cost terms (the kernel's form 1) -- TEST INFRASTRUCTURE ONLY.

main/planner/multi_trajectory_planner.py searches one scenario under every (e, p, o) of wh_ego x wh_policy x wh_other.  It is not
the generic planner (oracle/planner_oracle.py, main/lib/mp_search_ww_generic.py) with other numbers; it differs in three places:
  :185-201  heuristic   e * np.hypot(x - gx, y - gy) + p * |((theta - gtheta) + pi) % 2 pi - pi| + o * steering_change(node, goal)
                        (no obstacle and no centre term; the generic one has sqrt(dx^2 + dy^2) and min(|dtheta|, |dtheta| - tol / 2))
  :137-141  edge cost   the obstacle term is guarded by wc_obstacle != 0 (the generic file guards it by wh_obstacle != 0, :230), so
                        with the default wc_obstacle = 0.1 it is live in every search
  :141                  1 / d if d > 0 else inf
Everything else -- A*, collision test, poses, trajectory -- is PlannerOracle's."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import planner_oracle as PO                                          # noqa: E402


class MultiTrajectoryOracle(PO.PlannerOracle):
    """wh = (e, p, o, 0, 0): the weights of distance, heading difference and steering proxy; wc as in PlannerOracle."""

    def dist_obstacle(self, node):                                   # :162-177 (np.sqrt, `if dist < min_dist`)
        x0, y0 = node[0], node[1]
        best = float("inf")
        for hp in self.hp:
            d = min(abs(a * x0 + b * y0 + c) / np.sqrt(a ** 2 + b ** 2) for a, b, c in hp) if len(hp) else 0.0
            if d < best:
                best = d
        return best

    def heuristic(self, node):                                       # :185-201
        x, y, th = node
        gx, gy, gth = self.goal
        dist_xy = np.hypot(x - gx, y - gy)
        dth = abs(((th - gth) + np.pi) % (2 * np.pi) - np.pi)
        steer = self.steering_change(node, self.goal)
        return self.wh_dist * dist_xy + self.wh_theta * dth + self.wh_steer * steer

    def neighbors(self, node):                                       # :112-153
        mtx = PO.transform_mtx(*node)
        for k, (name, pts, total) in enumerate(self.mps):
            ccp = PO.transform_pts(node[2], mtx, self.cc[k])
            xy = ccp[:, :2].T
            if any(PO.check_collision(o, xy) for o in self.hp):
                continue
            x, y, th = tuple(np.squeeze(PO.transform_pts(node[2], mtx, np.atleast_2d(pts[-1]))).tolist())
            nb = (x, y, PO.normalize_angle(th))
            self.edge_mp[(node, nb)] = k
            steer = self.steering_change(node, nb)
            obst = 0.0
            center = 0.0
            if self.wc_obst != 0.0:
                d = self.dist_obstacle(nb)
                obst = (1.0 / d) if d > 0.0 else float("inf")
            if self.wc_center != 0.0:
                center = np.linalg.norm([x, y])
            yield self.wc_dist * total + self.wc_steer * steer + self.wc_obst * obst + self.wc_center * center, nb
