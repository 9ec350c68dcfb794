"""Host side of the pixel policy-evaluation tests: the episode slots of an evaluation rebuilt from
its per-step trace (numpy only, no GPU)."""
from types import SimpleNamespace

import numpy as np


def rebuild_slots(rew, done, episodes):
    """What ``rrl_pong_eval_step`` must have left after the traced steps ``rew`` / ``done`` [S, N]
    (cells of envs that did not step may hold anything: they are never read).

    An env steps while it has finished fewer than ``episodes`` episodes.  Returns ``ep_ret``
    (float64), ``ep_len``, ``ep_code`` [episodes, N] (unwritten slots: NaN / -1), ``ep_cnt`` [S, N] and
    ``remaining`` [S] after every step, ``active`` [S, N] (the env stepped) and ``points`` [episodes,
    N, 2]: the episode's -1 and +1 rewards.  Code 1: one of the two reached 21; else 2."""
    rew, done = np.asarray(rew, np.float64), np.asarray(done)
    S, N = rew.shape
    E = int(episodes)
    ep_ret = np.full((E, N), np.nan)
    ep_len = np.full((E, N), -1, np.int64)
    ep_code = np.full((E, N), -1, np.int64)
    points = np.zeros((E, N, 2), np.int64)
    ep_cnt = np.zeros((S, N), np.int64)
    remaining = np.zeros(S, np.int64)
    active = np.zeros((S, N), bool)
    cnt = np.zeros(N, np.int64)
    ret, ln = np.zeros(N), np.zeros(N, np.int64)
    lost, won = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for t in range(S):
        for e in np.flatnonzero(cnt < E):
            active[t, e] = True
            ret[e] += rew[t, e]
            ln[e] += 1
            lost[e] += rew[t, e] == -1
            won[e] += rew[t, e] == 1
            if done[t, e] > 0:
                k = cnt[e]
                ep_ret[k, e], ep_len[k, e] = ret[e], ln[e]
                ep_code[k, e] = 1 if max(lost[e], won[e]) >= 21 else 2
                points[k, e] = lost[e], won[e]
                cnt[e] += 1
                ret[e], ln[e], lost[e], won[e] = 0.0, 0, 0, 0
        ep_cnt[t] = cnt
        remaining[t] = int((cnt < E).sum())
    return SimpleNamespace(ep_ret=ep_ret, ep_len=ep_len, ep_code=ep_code, ep_cnt=ep_cnt, remaining=remaining,
                           active=active, points=points)
