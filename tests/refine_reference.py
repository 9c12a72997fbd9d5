"""The rule of include/lightdock_hip.h "Local refinement" in numpy and `math`, with the energy function passed in.

Every step is an IEEE add, multiply, divide or square root on doubles, so a device that follows the same rule gives the
same bits.  The start of the rotation step is `math.cos` / `math.sin`, the libm the library's host code calls; the quaternion
product is the oracle's `q_mul` (src/qt.rs:177-184).  State is a dict of per-pose arrays:

    energy, trans_step, rot_cos, rot_sin, nm_step   float64
    halvings, accepted, evaluations                 uint32
    frozen                                          uint8
"""
import math

import numpy as np

HALVED, FROZEN, NOT_EVALUATED = -1, -2, -3


def trial_count(pose_len):
    return 12 + 2 * (pose_len - 7)


def start_state(energy, trans_step, rot_step, nm_step):
    n = len(energy)
    return {"energy": np.array(energy, dtype=np.float64),
            "trans_step": np.full(n, trans_step, dtype=np.float64),
            "rot_cos": np.full(n, math.cos(rot_step / 2), dtype=np.float64),
            "rot_sin": np.full(n, math.sin(rot_step / 2), dtype=np.float64),
            "nm_step": np.full(n, nm_step, dtype=np.float64),
            "halvings": np.zeros(n, dtype=np.uint32), "accepted": np.zeros(n, dtype=np.uint32),
            "evaluations": np.ones(n, dtype=np.uint32), "frozen": np.zeros(n, dtype=np.uint8)}


def copy_state(state):
    return {k: v.copy() for k, v in state.items()}


def halve(state, p):
    """One failure below the limit: every step of pose p halves; the half angle's cosine and sine by the half-angle formulas."""
    state["halvings"][p] += 1
    state["trans_step"][p] = state["trans_step"][p] * 0.5
    state["nm_step"][p] = state["nm_step"][p] * 0.5
    c, s = state["rot_cos"][p], state["rot_sin"][p]
    with np.errstate(all="ignore"):
        c2 = np.sqrt((1.0 + c) * 0.5)
        state["rot_sin"][p] = s / (2.0 * c2)
    state["rot_cos"][p] = c2


def trial_row(q_mul, row, pose_len, j, dt, c, s, dn):
    """Trial j of one pose: a copy of `row` (its first pose_len doubles) with the move applied."""
    out = np.array(row[:pose_len], dtype=np.float64)
    sign = 1.0 if j % 2 == 0 else -1.0
    with np.errstate(all="ignore"):
        if j < 6:
            k = j // 2
            out[k] = out[k] + dt if sign > 0 else out[k] - dt
        elif j < 12:
            r = np.zeros(4)
            r[0] = c
            r[1 + (j - 6) // 2] = s if sign > 0 else -s
            out[3:7] = q_mul(r, out[3:7])
        else:
            m = 7 + (j - 12) // 2
            out[m] = out[m] + dn if sign > 0 else out[m] - dn
    return out


def trials(q_mul, poses, pose_len, state):
    """(n, K, pose_len) trial rows and (n, K) active bytes; a frozen pose's rows are left at zero and its bytes are 0."""
    n, K = poses.shape[0], trial_count(pose_len)
    rows = np.zeros((n, K, pose_len))
    active = np.zeros((n, K), dtype=np.uint8)
    for p in range(n):
        if state["frozen"][p]:
            continue
        active[p] = 1
        for j in range(K):
            rows[p, j] = trial_row(q_mul, poses[p], pose_len, j, state["trans_step"][p], state["rot_cos"][p],
                                   state["rot_sin"][p], state["nm_step"][p])
    return rows, active


def select(q_mul, poses, pose_len, state, energies, max_halvings, gaps=None):
    """One iteration's choice for every pose, in place; returns its history entries (int16).  energies: (n, K); a frozen
    pose's row is never read.  gaps (a list) receives the decision gap of every evaluated pose."""
    n, K = poses.shape[0], trial_count(pose_len)
    history = np.full(n, NOT_EVALUATED, dtype=np.int16)
    for p in range(n):
        if state["frozen"][p]:
            continue
        e = np.array(energies[p, :K], dtype=np.float64)
        e[np.isnan(e)] = -np.inf
        best = int(np.argmax(e))          # the first index of the maximum
        state["evaluations"][p] += K
        E = state["energy"][p]
        if e[best] > E:
            if gaps is not None:
                second = np.max(np.delete(e, best)) if K > 1 else -np.inf
                gaps.append(min(e[best] - second, e[best] - E))
            poses[p, :pose_len] = trial_row(q_mul, poses[p], pose_len, best, state["trans_step"][p], state["rot_cos"][p],
                                            state["rot_sin"][p], state["nm_step"][p])
            state["energy"][p] = e[best]
            state["accepted"][p] += 1
            history[p] = best
        else:
            if gaps is not None:
                gaps.append(E - e[best])
            if state["halvings"][p] < max_halvings:
                halve(state, p)
                history[p] = HALVED
            else:
                state["frozen"][p] = 1
                history[p] = FROZEN
    return history


def refine(q_mul, energy_fn, poses, pose_len, iterations, max_halvings, trans_step, rot_step, nm_step):
    """The whole loop.  energy_fn(rows (m, pose_len)) -> (m,) energies.  Returns the refined poses, the start and final
    energies, the final state, the history (n, iterations) and the smallest decision gap."""
    poses = np.array(poses, dtype=np.float64)
    n, K = poses.shape[0], trial_count(pose_len)
    before = np.asarray(energy_fn(np.ascontiguousarray(poses[:, :pose_len])), dtype=np.float64)
    state = start_state(before, trans_step, rot_step, nm_step)
    history = np.full((n, iterations), NOT_EVALUATED, dtype=np.int16)
    gaps = []
    for it in range(iterations):
        live = np.flatnonzero(state["frozen"] == 0)
        if live.size == 0:
            break
        rows, _ = trials(q_mul, poses, pose_len, state)
        energies = np.zeros((n, K))
        energies[live] = np.asarray(energy_fn(np.ascontiguousarray(rows[live].reshape(-1, pose_len)))).reshape(-1, K)
        history[:, it] = select(q_mul, poses, pose_len, state, energies, max_halvings, gaps)
    return {"poses": poses, "before": before, "after": state["energy"].copy(), "state": state, "history": history,
            "min_gap": min(gaps) if gaps else math.inf}
