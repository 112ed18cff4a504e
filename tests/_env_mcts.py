"""NumPy restatement of the network-free MCTS agent for det-MADN (TEST INFRASTRUCTURE ONLY): mctx muzero_policy whose
model is the environment itself, with random-rollout leaf values.

The reference has the construction (MADN/deterministic_madn.py:481-589 winning_action / policy_function / rollout /
value_function / root_fn / recurrent_fn, driven by MADN/simulate_deterministicMADN.py:12-35; TicTacToe/mcts.py:9-23 is
the same thing, live) but not a runnable path: rollout returns a shape-(4,) array (get_winner is bool[4]), the driver
lacks its imports, and recurrent_fn discounts by -1 even when the same side moves again (bonus turn on 6, passes).
Parity with the reference: UNPINNED.  This file is the definition; csrc/env_mcts.hip equals it bit for bit (all
values are in {-1, 0, 1}, the tree arithmetic is tests/_mctx_muzero.py's).

Built on oracle/detmadn.py (the environment) and tests/_mctx_muzero.py (Tree, action_scores, root_prior_logits,
final_draw: muzero_policy's pieces).  muzero_policy itself is not called, for two reasons: it masks at the root only,
where this agent masks every node's illegal actions the way the root mask works (FMIN before the softmax, score -inf);
and the rollout of simulation i is keyed by i, which a recurrent_fn is not told.

For a state s, side(p) = p % 2 with teams, else p:
  legal(s)    the 24-bit valid_action mask;  wins(s): bit a set iff a is legal and env_step(s, a) returns reward 1
  node mask   legal(s), 0 for a finished game; a node with mask 0 counts as all 24 actions legal
  prior       logits 100 legal + 200 wins, FMIN outside the node's mask
  transition  env_step, then no_step while the state is not done and has no legal action (at most MAX_PASSES times);
              reward env_step's; discount 0 if done, +1 if the side to move is the side that moved, else -1
              (a finished game stays as it is: reward 0, discount 0)
  value       0 if done; else the rollout: at most rollout_steps turns, each no_step without a legal action, else a
              uniform pick among wins if any, else among legal -- the k-th set bit, k = min(floor(u count), count - 1)
              in float32, u = rollout_uniform(seed, game, turn, node, rollout turn), node 0 the root and i + 1
              simulation i; +1 if the side to move at its start has won, -1 if another side has, 0 at the cap
  search      muzero_policy as csrc/puct_search.hip runs it; a root that is done or has no legal action is not searched
              (action -1, weights 0, value 0)."""
from __future__ import annotations

import json
import os

import numpy as np

from oracle import detmadn as dm
from oracle import mctx_stochastic as MS
from oracle.selfplay import M64, _mix64
from tests import _mctx_muzero as PZ

F32 = np.float32
A = 24
ALL = (1 << A) - 1
MAX_PASSES = 4
ROLLOUT_STREAM = 0x7011007D1CE      # csrc/env_mcts.hip kRolloutStream
ROOTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "env_mcts_roots.json")
RULE_SETS = {
    "default_2p": dict(num_players=2, **dm.DEFAULT_RULES),
    "selfplay_4p_teams": dict(num_players=4, **dm.SELFPLAY_RULES),
}


# ---- states ---------------------------------------------------------------------------------------------------------
def side(env, p):
    return int(p) % 2 if env.rules["enable_teams"] else int(p)


def legal_bits(env) -> int:
    va = dm.valid_action(env).flatten()
    return int(sum(1 << i for i in range(A) if va[i]))


def bits_to_bool(bits: int) -> np.ndarray:
    return ((int(bits) >> np.arange(A)) & 1).astype(bool)


def wins_trial(env, legal: int | None = None) -> int:
    """wins(s) by its definition: a trial env_step of every legal action."""
    legal = legal_bits(env) if legal is None else legal
    return sum(1 << a for a in range(A) if (legal >> a) & 1 and dm.env_step(env, dm.map_action(a))[1] == 1)


def wins_fast(env, legal: int | None = None) -> int:
    """wins(s) as the kernel forms it (csrc/env_mcts.hip det_wins_g): only the move that brings the mover's
    (substituted player's) last pin from the track onto one of its goal cells can complete its goal -- pins in the
    goal are never hit -- so: three pins on goal cells, env_step's landing cell of the fourth, and get_winner on the
    board with the mover's goal full."""
    legal = legal_bits(env) if legal is None else legal
    R = env.rules
    cp = dm._sub_player(env)
    goal = env.goal[cp].astype(np.int64)
    pins = env.pins[cp].astype(np.int64)
    in_goal = (pins >= goal[0]) & (pins <= goal[3])
    if legal == 0 or in_goal.sum() != 3:
        return 0
    i = int(np.flatnonzero(~in_goal)[-1])
    cur, target = int(pins[i]), int(env.target[cp])
    if cur == -1:
        return 0
    done = [dm.is_player_done(env.num_players, env.board, env.goal, p) for p in range(4)]
    done[cp] = True
    if R["enable_teams"]:
        t0, t1 = done[0] and done[2], done[1] and done[3]
        won = t0 != t1 and (t0 if cp % 2 == 0 else t1)
    else:
        won = True
    out = 0
    for m in range(1, 7):
        a = i * 6 + m - 1
        x = cur + m - target - int(R["must_traverse_start"])
        if not (legal >> a) & 1 or not (4 >= x > 0 and cur <= target):
            continue
        free = dm.check_goal_path_for_pin(-np.ones(4, np.int64), x, goal, env.board, cp)
        if int(env.board[int(dm._g(goal, x - 1))]) != cp and (R["enable_jump_in_goal_area"] or free) and won:
            out |= 1 << a
    return out


def node_mask(env) -> int:
    return 0 if env.done else legal_bits(env)


def transition(env, a: int):
    """(next state, reward, discount, passes) of action index a at a node."""
    if env.done:
        return env, 0, 0.0, 0
    nxt, reward, done = dm.env_step(env, dm.map_action(a))
    passes = 0
    while not nxt.done and passes < MAX_PASSES and legal_bits(nxt) == 0:
        nxt = dm.no_step(nxt)[0]
        passes += 1
    if done:
        disc = 0.0
    else:
        disc = 1.0 if side(nxt, nxt.current_player) == side(env, env.current_player) else -1.0
    return nxt, reward, disc, passes


def prior_logits(mask: int, wins: int) -> np.ndarray:
    """100 legal + 200 wins, FMIN outside the node's mask (mask 0: all 24 actions legal, logits 0)."""
    lg = (F32(100.0) * bits_to_bool(mask).astype(F32) + F32(200.0) * bits_to_bool(wins).astype(F32)).astype(F32)
    return np.where(bits_to_bool(mask if mask else ALL), lg, PZ.FMIN).astype(F32)


# ---- the rollout ----------------------------------------------------------------------------------------------------
def rollout_uniform(seed, gid, turn, node, step):
    """csrc/env_mcts.hip rollout: U[0,1) on a 24-bit grid, a stream of its own keyed by (seed, game, turn, node,
    rollout turn) -- never by lane or batch position."""
    key = ((seed ^ ROLLOUT_STREAM) & M64) ^ _mix64(((gid & 0xFFFFFFFF) << 32) | (turn & 0xFFFFFFFF))
    h = _mix64(key ^ _mix64(((node & 0xFFFFFFFF) << 16) | (step & 0xFFFFFFFF)))
    return F32((h >> 40) * (1.0 / 16777216.0))


def kth_set_bit(mask: int, u) -> int:
    cnt = bin(mask).count("1")
    k = min(int(F32(u) * F32(cnt)), cnt - 1)
    return int(np.flatnonzero(bits_to_bool(mask))[k])


def rollout(env, seed, gid, turn, node, steps, wins_fn=wins_fast):
    """-> (value seen from the side to move in env, turns played)."""
    side0 = side(env, env.current_player)
    turns = 0
    for i in range(steps):
        if env.done:
            break
        lm = legal_bits(env)
        if lm == 0:
            env = dm.no_step(env)[0]
        else:
            wm = wins_fn(env, lm)
            a = kth_set_bit(wm if wm else lm, rollout_uniform(seed, gid, turn, node, i))
            env = dm.env_step(env, dm.map_action(a))[0]
        turns += 1
    w = dm.get_winner(env, env.board)
    if any(w[p] and side(env, p) == side0 for p in range(4)):
        return F32(1.0), turns
    return F32(-1.0 if w.any() else 0.0), turns


# ---- the search -----------------------------------------------------------------------------------------------------
def search_one(env, S, D, temperature, rollout_steps, seed, turn, gid, dirichlet, gumbel, qtransform=PZ.QT_MIN_MAX,
               min_value=-1.0, max_value=1.0, dirichlet_fraction=0.0, pb_c_init=1.25, pb_c_base=19652.0):
    """One game's search -> dict(action, weights, value, visits, qvalues, turns, tree) (tree None when not searched)."""
    lm = node_mask(env)
    if lm == 0:
        return dict(action=-1, weights=np.zeros(A, F32), value=F32(0), visits=np.zeros(A, np.int32),
                    qvalues=np.zeros(A, F32), turns=0, tree=None)
    wm = wins_fast(env, lm)
    logits = (F32(100.0) * bits_to_bool(lm).astype(F32) + F32(200.0) * bits_to_bool(wm).astype(F32)).astype(F32)
    prior = PZ.root_prior_logits(logits[None], ~bits_to_bool(lm)[None], np.asarray(dirichlet, F32)[None],
                                 dirichlet_fraction)[0]
    value, turns = rollout(env, seed, gid, turn, 0, rollout_steps)
    t = PZ.Tree(S + 1, A, 1)
    t.update_node(0, prior, value, 0.0)
    states, masks = [env] + [None] * S, [lm] + [0] * S
    for sim in range(S):
        node, depth = 0, 0
        while True:                                   # search.py simulate, every node masked
            tb = [MS.tiebreak_uniform(seed, gid, turn, sim, depth, a) for a in range(A)]
            invalid = ~bits_to_bool(masks[node] if masks[node] else ALL)
            score, _ = PZ.action_scores(t, node, 0, invalid, tb, qtransform, min_value, max_value, pb_c_init, pb_c_base)
            a = int(np.argmax(score))
            nxt = int(t.c_index[node, a])
            depth += 1
            if nxt == -1 or depth >= D:
                break
            node = nxt
        nn = sim + 1 if nxt == -1 else nxt
        s2, r, d, _ = transition(states[node], a)       # search.py expand: recurrent_fn is the environment
        m2 = node_mask(s2)
        v = F32(0)
        if not s2.done:
            v, n = rollout(s2, seed, gid, turn, sim + 1, rollout_steps)
            turns += n
        t.update_node(nn, prior_logits(m2, wins_fast(s2, m2) if m2 else 0), v, 0.0)
        states[nn], masks[nn] = s2, m2
        t.c_index[node, a], t.c_reward[node, a], t.c_disc[node, a] = nn, F32(r), F32(d)
        t.parent[nn], t.afp[nn] = node, a
        idx = nn                                       # search.py backward
        leaf = F32(t.value[idx])
        while idx != 0:
            p = t.parent[idx]
            cnt = t.visits[p]
            pa = t.afp[idx]
            leaf = F32(t.c_reward[p, pa] + F32(t.c_disc[p, pa] * leaf))
            t.value[p] = F32(F32(F32(t.value[p] * F32(cnt)) + leaf) / (F32(cnt) + F32(1.0)))
            t.visits[p] = cnt + 1
            t.c_value[p, pa] = t.value[idx]
            t.c_visits[p, pa] += 1
            idx = p
    action, weights, _ = PZ.final_draw(t.c_visits[0], gumbel, temperature)
    return dict(action=action, weights=weights, value=F32(t.value[0]), visits=t.c_visits[0].copy(),
                qvalues=t.qvalues(0), turns=turns, tree=t)


def env_muzero_policy(envs, S, D, temperature, rollout_steps, seed, turn, gids=None, dirichlet=None, gumbel=None, **kw):
    """The batch: per-game searches stacked -> dict of arrays (action [B], weights / visits / qvalues [B, 24], value
    [B], turns [B]).  dirichlet / gumbel [B, 24] (zeros when left out: fraction 0 / an argmax of the visit logits)."""
    B = len(envs)
    gids = np.arange(B) if gids is None else np.asarray(gids)
    dirichlet = np.zeros((B, A), F32) if dirichlet is None else dirichlet
    gumbel = np.zeros((B, A), F32) if gumbel is None else gumbel
    rs = [search_one(e, S, D, temperature, rollout_steps, seed, turn, int(gids[b]), dirichlet[b], gumbel[b], **kw)
          for b, e in enumerate(envs)]
    return {k: np.stack([np.asarray(r[k]) for r in rs]) for k in ("action", "weights", "value", "visits", "qvalues",
                                                                  "turns")}


# ---- the fixture's root states --------------------------------------------------------------------------------------
def state_from_record(rule_set: str, rec: dict) -> dm.State:
    env = dm.env_reset(**RULE_SETS[rule_set])
    pins = np.asarray(rec["pins"], np.int8)
    return env.replace(pins=pins, board=dm.set_pins_on_board(env.board, pins),
                       action_set=np.asarray(rec["action_set"], np.int8), current_player=int(rec["current_player"]),
                       done=bool(rec["done"]), reward=int(rec["reward"]))


def load_roots(rule_set: str):
    """-> (oracle states, their tag lists) of one rule set of tests/golden/env_mcts_roots.json."""
    with open(ROOTS) as fh:
        recs = json.load(fh)[rule_set]
    return [state_from_record(rule_set, r) for r in recs], [r["tags"] for r in recs]


def device_state(E, rule_set: str, envs):
    """The oracle states as one detmadn.DetMADNState on the GPU."""
    kw = RULE_SETS[rule_set]
    rules = E.make_rules(**kw)
    return E.state_from_host(np.stack([e.pins for e in envs]), [e.current_player for e in envs], rules,
                             action_set=np.stack([e.action_set for e in envs]), done=[e.done for e in envs],
                             reward=[e.reward for e in envs])
