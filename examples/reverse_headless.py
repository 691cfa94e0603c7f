"""Reverse parking in the manner of the reference's example/reverse (`MPC(..., enable_reverse=True)` on a path whose fourth row is the gear): a car drives
forward past a bay between two boxes, backs into it and drives out forward again - run without a simulator window, twice:

  1. as the user's loop, `MPC.control` + the kinematic step per tick (the path's pieces are uploaded one by one as they come into force)
  2. as ONE `Fleet.rollout(..., gears=True)` of a small fleet of such cars on lanes of their own: every tick, the switch from piece to piece and the
     arrival rule on the device, one host wait

    python examples/reverse_headless.py [members]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from rda_planner_amd import scenarios as sc
from rda_planner_amd.fleet import Fleet
from rda_planner_amd.mpc import MPC

MPC_KW = dict(receding=10, iter_num=2, max_edge_num=4, max_obs_num=4, enable_reverse=True, goal_index_threshold=1)
DT, SPEED = 0.1, 3.0


def box(cx, cy, length, width):
    v = np.array([[cx - length / 2, cx + length / 2, cx + length / 2, cx - length / 2], [cy - width / 2, cy - width / 2, cy + width / 2, cy + width / 2]])
    return sc.Obstacle(None, None, v, "Rpositive", np.zeros((2, 1)))


def parking(lane=0, forward=6.0, back=4.0, out=5.0):
    """lane `lane`: the car, its path (forward `forward` m, back `back` m into the bay, `out` m forward again), the two boxes beside the bay, the start"""
    y = 10.0 * lane
    x0, x1 = 4.0, 4.0 + forward
    x2 = x1 - back
    path = sc.gear_path([((x0, y), (x1, y), 1), ((x1, y), (x2, y), -1), ((x2, y), (x2 + out, y), 1)], 0.1)
    boxes = [box(x2 + 1.0, y + 3.0, 5.0, 1.6), box(x2 + 1.0, y - 3.0, 5.0, 1.6)]
    return sc.rectangle_robot(dynamics="acker"), path, boxes, path[0][0:3].copy()


def hold_arrived(mpc):
    """a member that has arrived stays at the end of its last piece (`MPC._end` leaves `curve_index` past the last piece)"""
    mpc.curve_index, mpc.cur_index = len(mpc.curve_list) - 1, len(mpc.curve_list[-1]) - 1


def control_loop(steps=150):
    car, path, boxes, state = parking()
    mpc = MPC(car, path, sample_time=DT, **MPC_KW)
    t0, pieces, min_clear = time.perf_counter(), [], float("inf")
    for k in range(steps):
        pieces.append(mpc.curve_index)
        u, info = mpc.control(state, SPEED, boxes)
        state = sc.kinematic_step(state, u, car, DT)
        min_clear = min(min_clear, sc.clearance(car, state, boxes))
        if info["arrive"]:
            print(f"MPC.control loop: arrived after {k + 1} ticks")
            break
    dt = time.perf_counter() - t0
    switches = [k for k in range(1, len(pieces)) if pieces[k] != pieces[k - 1]]
    print(f"MPC.control loop: {len(pieces)} ticks, {len(pieces) / dt:.0f} ticks/s, pieces change at ticks {switches}, min clearance {min_clear:.2f} m")
    return np.asarray(state, float).ravel()


def fleet_rollout(members=3, steps=150):
    made = [parking(lane) for lane in range(members)]
    fleet = Fleet([MPC(car, path, sample_time=DT, **MPC_KW) for car, path, _, _ in made])
    t0 = time.perf_counter()
    out = fleet.rollout([m[3] for m in made], SPEED, steps, obstacle_lists=[m[2] for m in made], gears=True, moving=True, clearance=True)
    dt = time.perf_counter() - t0
    for i in range(members):
        switches = [int(k) for k in np.nonzero(np.diff(out["piece"][:, i]))[0] + 1]
        print(f"Fleet.rollout member {i}: pieces change at ticks {switches}, arrived at tick {int(out['arrived_at'][i])}, "
              f"min clearance {out['clearance'][:, i].min():.2f} m")
    print(f"Fleet.rollout(gears=True): {members} members x {steps} ticks in {1e3 * dt:.1f} ms, {members * steps / dt:.0f} ego-ticks/s")
    fleet.close()
    return out["states"][-1, 0]


def main():
    members = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    end_loop = control_loop()
    end_roll = fleet_rollout(members)
    print(f"end state of the loop {np.round(end_loop, 4)} and of member 0 of the rollout {np.round(end_roll, 4)}")


if __name__ == "__main__":
    main()
