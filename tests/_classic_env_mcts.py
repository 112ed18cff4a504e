"""NumPy restatement of the network-free MCTS agent for classic (dice) MADN (TEST INFRASTRUCTURE ONLY): mctx
stochastic_muzero_policy whose model is the environment itself, with random-rollout leaf values.

The reference sketches the construction (MADN/classic_madn.py:543-714 winning_action / policy_function / rollout /
value_function / recurrent_chance_fn / recurrent_fn / root_fn, meant for mctx.stochastic_muzero_policy) but the path
cannot run: winning_action builds its state without `key` (SURVEY.md row 2b calls it a broken demo path), its discounts
never change sign between sides, and its chance logits are uniform even where the environment rethrows a soft-locked
player's die.  Parity with the reference: UNPINNED.  This file is the definition; csrc/classic_env_mcts.hip equals it
bit for bit (values are in {-1, 0, 1}, priors are 0, 1/k or the die tables, the tree arithmetic is restated operation
by operation).

Built on oracle/classic_madn.py (states, dice_probabilities, choice_from_uniform, env_step, no_step, set_die),
oracle/mctx_stochastic.py (_Tree with its A' = 4 + 6 child slots and info = (reward, discount),
qtransform_by_parent_and_siblings, tiebreak_uniform), tests/_mctx_muzero.py (log_cr, root_prior_logits' steps,
final_draw) and tests/_env_mcts.py (side, kth_set_bit).  stochastic_muzero_policy itself is not called: it masks at the
root only, softmaxes the stored logits on every visit (here a node keeps its prior probabilities, the chance nodes the
environment's own numbers with no log / softmax round trip), and the rollout of simulation i is keyed by i, which a
recurrent_fn is not told.

side(p) = p % 2 with teams, else p.
  root        a state whose die is thrown; done, or without a legal pin for its die: not searched (action -1, weights
              0, value 0)
  decision    mask valid_action (4 bits); prior softmax of 100 legal + 200 wins with FMIN outside the mask (wins: pin
              legal and env_step returns reward 1); a non-root decision node that is done or has no legal pin has
              exactly one action, pin 0, which applies no_step
  -> chance   afterstate = env_step / no_step; edge reward 0, discount 1; info = (reward, discount): env_step's reward
              (0 for no_step); 0 if done, +1 if side(next to move) == side(mover), else -1
  chance      child priors dice_probabilities(afterstate); selection argmax p[c] / (n[c] + 1); value: a rollout from
              the afterstate seen from the side that MOVED.  Of a finished afterstate the value is info's reward: the
              +1 the mover's side has just won (what a zero-turn rollout returns: "+1 if the viewing side has won").
              The stochastic wrapper pays the step's reward on the chance -> decision edges, so only with this value
              does every backup through a won afterstate carry 1 and a winning pin's q-value equal 1.0 exactly (with 0
              it would be (n - 1) / n after n visits)
  -> decision state = set_die(afterstate, c + 1); edge reward / discount = the chance node's info; value 0 if done, else
              a rollout seen from the side to move
  rollout     at most rollout_steps turns: throw the die with choice_from_uniform(dice_probabilities, u0) (the first
              turn of a decision node's rollout keeps the node's die), then no_step without a legal pin, else a uniform
              pick among wins if any, else among legal -- the k-th set bit, k = min(floor(u1 count), count - 1); u0 /
              u1 = rollout_uniform(seed, game, turn, node, 2 t / 2 t + 1), node 0 the root and i + 1 simulation i; +1
              if the viewing side has won, -1 if another side has, 0 at the cap
  search      PUCT with qtransform_by_parent_and_siblings over the A' slots, the 1e-7 tie-break, pb_c as
              csrc/puct_search.hip; action weights = root visit fractions; root value clipped to [-1, 1]."""
from __future__ import annotations

import json
import os

import numpy as np

from oracle import classic_madn as cm
from oracle import mctx_gumbel as G
from oracle import mctx_stochastic as MS
from oracle.detmadn import check_goal_path_for_pin, _g, get_winner, is_player_done, set_pins_on_board
from oracle.selfplay import M64, _mix64
from tests import _mctx_muzero as PZ
from tests._env_mcts import kth_set_bit, side

F32 = np.float32
A, C = 4, 6
AP = A + C
ROLLOUT_STREAM = 0xC1A551CD1CE      # csrc/classic_env_mcts.hip kClassicRolloutStream
ROOTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "classic_env_mcts_roots.json")
RULE_SETS = {
    "selfplay_4p_teams": dict(num_players=4, **cm.SELFPLAY_RULES),
    "default_2p": dict(num_players=2, **cm.DEFAULT_RULES),
    "rethrow_six_2p": dict(num_players=2, **{**cm.DEFAULT_RULES, "enable_dice_rethrow": True,
                                            "enable_start_on_1": False}),
}


# ---- states ---------------------------------------------------------------------------------------------------------
def legal_bits(env) -> int:
    va = cm.valid_action(env)
    return int(sum(1 << i for i in range(A) if va[i]))


def wins_trial(env, legal: int | None = None) -> int:
    """wins(s) by its definition: a trial env_step of every legal pin."""
    legal = legal_bits(env) if legal is None else legal
    return sum(1 << a for a in range(A) if (legal >> a) & 1 and cm.env_step(env, a)[1] == 1)


def wins_fast(env, legal: int | None = None) -> int:
    """wins(s) as the kernel forms it (csrc/classic_env_mcts.hip cls_wins): only the move that brings the mover's
    (substituted player's) last pin from the track onto one of its goal cells can complete its goal -- pins in the
    goal are never hit -- so: three pins on goal cells, env_step's landing cell of the fourth, and get_winner on the
    board with the mover's goal full."""
    legal = legal_bits(env) if legal is None else legal
    R = env.rules
    cp = cm._sub_player(env)
    goal = env.goal[cp].astype(np.int64)
    pins = env.pins[cp].astype(np.int64)
    in_goal = (pins >= goal[0]) & (pins <= goal[3])
    if in_goal.sum() != 3:
        return 0
    i = int(np.flatnonzero(~in_goal)[-1])
    cur, target = int(pins[i]), int(env.target[cp])
    if not (legal >> i) & 1 or cur == -1:
        return 0
    x = cur + int(env.die) - target - int(R["must_traverse_start"])
    if not (4 >= x > 0 and cur <= target):
        return 0
    free = check_goal_path_for_pin(-np.ones(4, np.int64), x, goal, env.board, cp)
    if int(env.board[int(_g(goal, x - 1))]) == cp or not (R["enable_jump_in_goal_area"] or free):
        return 0
    done = [is_player_done(env.num_players, env.board, env.goal, p) for p in range(4)]
    done[cp] = True
    if R["enable_teams"]:
        t0, t1 = done[0] and done[2], done[1] and done[3]
        won = t0 != t1 and (t0 if cp % 2 == 0 else t1)
    else:
        won = True
    return (1 << i) if won else 0


def decision_step(env, pin: int, passing: bool):
    """recurrent_fn: (afterstate, reward, discount) of pin `pin` at a decision node (passing: no_step)."""
    if passing:
        nxt, reward = cm.no_step(env)[0], 0
    else:
        nxt, reward, _ = cm.env_step(env, pin)
    if nxt.done:
        disc = 0.0
    else:
        disc = 1.0 if side(nxt, nxt.current_player) == side(env, env.current_player) else -1.0
    return nxt, int(reward), disc


def chance_priors(after) -> np.ndarray:
    """A chance node's six child priors: the environment's own numbers."""
    return np.asarray(cm.dice_probabilities(after), F32)


def softmax4(x) -> np.ndarray:
    """Softmax over the 4 pins in the device's order: exp correctly rounded, the sum (e0 + e1) + (e2 + e3)
    (csrc/tree.hpp row_softmax24 with lanes 4.. empty)."""
    x = np.asarray(x, F32)
    with np.errstate(over="ignore"):
        e = G.exp_cr((x - x.max()).astype(F32)).astype(F32)
    s = F32(F32(e[0] + e[1]) + F32(e[2] + e[3]))
    return (e / s).astype(F32)


def decision_prior(mask: int, wins: int) -> np.ndarray:
    """softmax of 100 legal + 200 wins inside the node's mask, FMIN outside."""
    bits = np.array([(mask >> a) & 1 for a in range(A)], bool)
    w = np.array([(wins >> a) & 1 for a in range(A)], bool)
    lg = (F32(100.0) * bits.astype(F32) + F32(200.0) * w.astype(F32)).astype(F32)
    return softmax4(np.where(bits, lg, PZ.FMIN).astype(F32))


def root_prior(mask: int, wins: int, dirichlet, dirichlet_fraction) -> np.ndarray:
    """_add_dirichlet_noise, _get_logits_from_probs, _mask_invalid_actions on the unmasked 100 legal + 200 wins, then
    the probabilities the root keeps."""
    bits = np.array([(mask >> a) & 1 for a in range(A)], bool)
    w = np.array([(wins >> a) & 1 for a in range(A)], bool)
    f = F32(dirichlet_fraction)
    probs = softmax4((F32(100.0) * bits.astype(F32) + F32(200.0) * w.astype(F32)).astype(F32))
    noisy = ((F32(1.0) - f) * probs + f * np.asarray(dirichlet, F32)).astype(F32)
    logits = PZ.log_cr(np.maximum(noisy, F32(PZ.TINY)))
    logits = (logits - logits.max()).astype(F32)
    return softmax4(np.where(bits, logits, PZ.FMIN).astype(F32))


# ---- the rollout ----------------------------------------------------------------------------------------------------
def rollout_uniform(seed, gid, turn, node, j):
    """csrc/classic_env_mcts.hip rollout_u: U[0,1) on a 24-bit grid, a stream of its own keyed by (seed, game, turn,
    node, draw) -- never by lane or batch position."""
    key = ((seed ^ ROLLOUT_STREAM) & M64) ^ _mix64(((gid & 0xFFFFFFFF) << 32) | (turn & 0xFFFFFFFF))
    h = _mix64(key ^ _mix64(((node & 0xFFFFFFFF) << 16) | (j & 0xFFFFFFFF)))
    return F32((h >> 40) * (1.0 / 16777216.0))


def rollout(env, view, seed, gid, turn, node, steps, keep_die, wins_fn=wins_fast):
    """-> (value seen from side `view`, turns played)."""
    turns = 0
    for t in range(steps):
        if env.done:
            break
        if t > 0 or not keep_die:
            env = cm.set_die(env, cm.choice_from_uniform(cm.dice_probabilities(env),
                                                         rollout_uniform(seed, gid, turn, node, 2 * t)))
        lm = legal_bits(env)
        if lm == 0:
            env = cm.no_step(env)[0]
        else:
            wm = wins_fn(env, lm)
            env = cm.env_step(env, kth_set_bit(wm if wm else lm, rollout_uniform(seed, gid, turn, node, 2 * t + 1)))[0]
        turns += 1
    w = get_winner(env, env.board)
    if any(w[p] and side(env, p) == view for p in range(4)):
        return F32(1.0), turns
    return F32(-1.0 if w.any() else 0.0), turns


# ---- the search -----------------------------------------------------------------------------------------------------
def decision_scores(t, n, mask, tb, pb_c_init, pb_c_base):
    """muzero_action_selection's to_argmax over the A' slots: -inf outside the node's mask (the chance slots too)."""
    vs = MS.qtransform_by_parent_and_siblings(t, n)
    nv = F32(t.visits[n])
    pb_c = F32(F32(pb_c_init) + PZ.log_cr(F32(F32(nv + F32(pb_c_base) + F32(1.0)) / F32(pb_c_base))))
    c = F32(np.sqrt(nv) * pb_c)
    ps = (c * t.c_prior[n] / (t.c_visits[n] + 1).astype(F32)).astype(F32)
    score = (vs + ps + F32(1e-7) * np.asarray(tb, F32)).astype(F32)
    ok = np.array([a < A and (mask >> a) & 1 for a in range(AP)], bool)
    return np.where(ok, score, -np.inf)


def chance_scores(t, n):
    x = (t.c_prior[n, A:] / (t.c_visits[n, A:] + 1).astype(F32)).astype(F32)
    return np.concatenate([np.full(A, -np.inf), x])


def search_one(env, S, D, temperature, rollout_steps, seed, turn, gid, dirichlet, gumbel, dirichlet_fraction=0.0,
               pb_c_init=1.25, pb_c_base=19652.0):
    """One game's search -> dict(action, weights, value, visits, qvalues, turns, tree, states, passing) (tree None
    when not searched)."""
    lm = 0 if env.done else legal_bits(env)
    if lm == 0:
        return dict(action=-1, weights=np.zeros(A, F32), value=F32(0), visits=np.zeros(A, np.int32),
                    qvalues=np.zeros(A, F32), turns=0, tree=None)
    no_emb = np.zeros(0, F32)
    t = MS._Tree(S + 1, AP, 0)
    prior = np.concatenate([root_prior(lm, wins_fast(env, lm), dirichlet, dirichlet_fraction), np.zeros(C, F32)])
    value, turns = rollout(env, side(env, env.current_player), seed, gid, turn, 0, rollout_steps, True)
    t.update_node(0, prior, value, True, no_emb, (0.0, 0.0))
    states, masks, passing = [env] + [None] * S, [lm] + [0] * S, [False] * (S + 1)
    for sim in range(S):
        node, depth = 0, 0
        while True:                                   # search.py simulate
            if t.is_dec[node]:
                tb = [MS.tiebreak_uniform(seed, gid, turn, sim, depth, a if a < A else 0) for a in range(AP)]
                score = decision_scores(t, node, masks[node], tb, pb_c_init, pb_c_base)
            else:
                score = chance_scores(t, node)
            a = int(np.argmax(score))
            nxt = int(t.c_index[node, a])
            depth += 1
            if nxt == -1 or depth >= D:
                break
            node = nxt
        nn = sim + 1 if nxt == -1 else nxt
        s = states[node]
        if t.is_dec[node]:                            # recurrent_fn: the afterstate
            s2, r, d = decision_step(s, a, passing[node])
            mover = side(s, s.current_player)
            v = F32(r)
            if not s2.done:
                v, n = rollout(s2, mover, seed, gid, turn, sim + 1, rollout_steps, False)
                turns += n
            t.update_node(nn, np.concatenate([np.zeros(A, F32), chance_priors(s2)]), v, False, no_emb, (r, d))
            er, ed = F32(0.0), F32(1.0)
            masks[nn], passing[nn] = 0, False
        else:                                         # recurrent_chance_fn: the die
            s2 = cm.set_die(s, a - A + 1)
            m2 = 0 if s2.done else legal_bits(s2)
            v = F32(0)
            if not s2.done:
                v, n = rollout(s2, side(s2, s2.current_player), seed, gid, turn, sim + 1, rollout_steps, True)
                turns += n
            passing[nn] = m2 == 0
            masks[nn] = m2 if m2 else 1
            t.update_node(nn, np.concatenate([decision_prior(masks[nn], wins_fast(s2, m2) if m2 else 0),
                                              np.zeros(C, F32)]), v, True, no_emb, (0.0, 0.0))
            er, ed = F32(t.info[node, 0]), F32(t.info[node, 1])
        states[nn] = s2
        t.c_index[node, a], t.c_reward[node, a], t.c_disc[node, a] = nn, er, ed
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
    action, weights, _ = PZ.final_draw(t.c_visits[0, :A], gumbel, temperature)
    return dict(action=action, weights=weights, value=F32(np.clip(t.value[0], -1.0, 1.0)),
                visits=t.c_visits[0, :A].copy(), qvalues=t.qvalues(0)[:A].copy(), turns=turns, tree=t, states=states,
                passing=passing)


def env_stochastic_muzero_policy(envs, S, D, temperature, rollout_steps, seed, turn, gids=None, dirichlet=None,
                                 gumbel=None, **kw):
    """The batch: per-game searches stacked -> dict of arrays (action [B], weights / visits / qvalues [B, 4], value
    [B], turns [B]).  dirichlet / gumbel [B, 4] (zeros when left out: fraction 0 / an argmax of the visit logits)."""
    B = len(envs)
    gids = np.arange(B) if gids is None else np.asarray(gids)
    dirichlet = np.zeros((B, A), F32) if dirichlet is None else dirichlet
    gumbel = np.zeros((B, A), F32) if gumbel is None else gumbel
    rs = [search_one(e, S, D, temperature, rollout_steps, seed, turn, int(gids[b]), dirichlet[b], gumbel[b], **kw)
          for b, e in enumerate(envs)]
    return {k: np.stack([np.asarray(r[k]) for r in rs]) for k in ("action", "weights", "value", "visits", "qvalues",
                                                                  "turns")}


# ---- the fixture's root states --------------------------------------------------------------------------------------
def state_from_record(rule_set: str, rec: dict) -> cm.State:
    env = cm.env_reset(**RULE_SETS[rule_set])
    pins = np.asarray(rec["pins"], np.int8)
    return env.replace(pins=pins, board=set_pins_on_board(-np.ones_like(env.board), pins),
                       current_player=int(rec["current_player"]), done=bool(rec["done"]), reward=int(rec["reward"]),
                       die=int(rec["die"]))


def load_roots(rule_set: str):
    """-> (oracle states, their tag lists) of one rule set of tests/golden/classic_env_mcts_roots.json."""
    with open(ROOTS) as fh:
        recs = json.load(fh)[rule_set]
    return [state_from_record(rule_set, r) for r in recs], [r["tags"] for r in recs]


def device_state(E, rule_set: str, envs):
    """The oracle states as one classic.ClassicMADNState on the GPU."""
    rules = E.make_rules(**RULE_SETS[rule_set])
    return E.state_from_host(np.stack([e.pins for e in envs]), [e.current_player for e in envs], rules,
                             die=[e.die for e in envs], done=[e.done for e in envs], reward=[e.reward for e in envs])
