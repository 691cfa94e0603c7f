"""What the tracker's tests share (tests/test_lidar_track.py, tests/test_gpu_lidar_track.py): crafted box sequences and the crossing scene."""
import numpy as np

from rda_planner_amd import scenarios as sc

DT, SPEED = 0.1, 4.0
T, N, E, ITER, MARGIN = 12, 4, 4, 2, 3
TICKS, EPS, MINS = 40, 2.0, 4
UNIT = np.array([[-1.0, -1.0], [1.0, -1.0], [1.0, 1.0], [-1.0, 1.0]])          # a 2 x 2 m box about its centre, counter-clockwise


def boxes_at(centres):
    """(n, 4, 2) boxes of 2 x 2 m about the (n, 2) centres"""
    return np.asarray(centres, float).reshape(-1, 1, 2) + UNIT[None]


def rigid_sequence(ticks, n=5, step=(0.25, -0.125), seed=3):
    """`ticks` ticks of n boxes that translate rigidly by `step` per tick, presented in another order every tick; centres and step are multiples of 1/8,
    so centres, differences and (with dt = 1/8 and an age of up to 8) the velocities are exact in doubles -> ([boxes (n, 4, 2)], [permutation])"""
    rng = np.random.default_rng(seed)
    base = np.array([[8.0 * (i % 3), 8.0 * (i // 3)] for i in range(n)]) + rng.integers(0, 16, (n, 2)) / 8.0
    out, perms = [], []
    for k in range(ticks):
        perm = rng.permutation(n)
        out.append(boxes_at(base + k * np.asarray(step))[perm])
        perms.append(perm)
    return out, perms


def crossing(lane):
    """Lane 0: a differential robot (4.6 x 1.6 m) drives at 4 m/s along y = 20 from x = 0; a 2 x 2 m box starts at (12, 14.5) and crosses the lane
    upwards at 2 m/s: its centre is on the lane after 2.75 s, when the robot's is at x = 11.  Lane 1 is the mirror image about y = 40: y = 60, the box
    from (12, 65.5) at -2 m/s.
    -> (car, path, the box as an obstacle with its velocity, the sensor: a full turn of 360 beams that sees 10 m)"""
    y, side = (20.0, -1.0) if lane == 0 else (60.0, 1.0)
    car = sc.rectangle_robot(dynamics="diff", wheelbase=0)
    path = sc.line_path([0, y, 0], [30, y, 0], 0.1)
    box = sc.box(12.0, y + side * 5.5, 2.0, 2.0, 0.0, velocity=(0.0, -side * 2.0))
    sensor = dict(number=360, angle_min=-np.pi, angle_max=np.pi, range_min=0.0, range_max=10.0)
    return car, path, box, sensor
