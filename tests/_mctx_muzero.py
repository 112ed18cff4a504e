"""NumPy restatement of mctx 0.0.6 ``muzero_policy`` on det-MADN (TEST INFRASTRUCTURE ONLY).

The reference keeps this call commented beside the Gumbel one (MuZero_det_MADN/muzero_deterministic_madn.py:685-697:
PUCT, qtransform_by_min_max(-1, 1), Dirichlet 0.25 / 0.3, temperature); mctx is not vendored, so this restates its
published algorithm from the oracle's helpers:
  mctx/_src/policies.py          muzero_policy, _add_dirichlet_noise, _get_logits_from_probs, _mask_invalid_actions,
                                 _apply_temperature
  mctx/_src/action_selection.py  muzero_action_selection
  mctx/_src/qtransforms.py       qtransform_by_min_max, qtransform_by_parent_and_siblings
  mctx/_src/search.py            search, simulate, expand, backward (as oracle/mctx_gumbel.py restates them)
Parity vs mctx itself: UNPINNED (no reference test covers it).

Randomness is explicit, as in oracle/mctx_stochastic.py: ``dirichlet`` [B, A] the root noise sample, ``gumbel`` [B, A]
the Gumbel draws of the final categorical, the 1e-7 tie-break uniforms from the engine's counter RNG
(mctx_stochastic.tiebreak_uniform).

The arithmetic is the device kernel's (csrc/puct_search.hip), so that with identical network outputs the two compare
bit for bit: float32 throughout, no fused multiply-add, sums over the actions in numpy's pairwise order
(mctx_gumbel.row_sum), exp and log correctly rounded (evaluated in float64 and rounded once: exp_cr, log_cr), sqrt and
division correctly rounded (numpy's float32 ones are), products left to right."""
from __future__ import annotations

import numpy as np

from oracle import mctx_gumbel as G
from oracle import mctx_stochastic as MS

F32 = np.float32
FMIN = G.FMIN
TINY = G.TINY
QT_MIN_MAX, QT_PARENT_SIBLINGS = "min_max", "parent_and_siblings"


def log_cr(x):
    """float32 log, correctly rounded: evaluated in float64 and rounded once (csrc/tree.hpp log_cr)."""
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(x, F32).astype(np.float64)).astype(F32)


def softmax(x):
    """Softmax of one row [A] in the device's order (mctx_gumbel.softmax: exp_cr, row_sum)."""
    return G.softmax(np.asarray(x, F32)[None])[0]


class Tree:
    """One game's tree (the field names mctx_stochastic.qtransform_by_parent_and_siblings reads)."""

    def __init__(self, N, A, L):
        self.visits = np.zeros(N, np.int32)
        self.value = np.zeros(N, F32)
        self.emb = np.zeros((N, L), F32)
        self.parent = np.full(N, -1, np.int32)
        self.afp = np.full(N, -1, np.int32)
        self.c_index = np.full((N, A), -1, np.int32)
        self.c_prior = np.zeros((N, A), F32)
        self.c_value = np.zeros((N, A), F32)
        self.c_visits = np.zeros((N, A), np.int32)
        self.c_reward = np.zeros((N, A), F32)
        self.c_disc = np.zeros((N, A), F32)

    def qvalues(self, n):
        return (self.c_reward[n] + self.c_disc[n] * self.c_value[n]).astype(F32)

    def update_node(self, n, prior, value, emb):
        self.c_prior[n] = prior
        self.value[n] = value
        self.visits[n] += 1
        self.emb[n] = emb


def qtransform_by_min_max(t: Tree, n, min_value, max_value):
    q = t.qvalues(n)
    lo, hi = F32(min_value), F32(max_value)
    return ((np.where(t.c_visits[n] > 0, q, lo) - lo) / F32(hi - lo)).astype(F32)


def puct_policy_score(t: Tree, n, pb_c_init=1.25, pb_c_base=19652.0):
    """sqrt(N) * pb_c * softmax(prior) / (visits + 1), evaluated left to right."""
    nv = F32(t.visits[n])
    pb_c = F32(F32(pb_c_init) + log_cr(F32(F32(nv + F32(pb_c_base) + F32(1.0)) / F32(pb_c_base))))
    c = F32(np.sqrt(nv) * pb_c)
    return (c * softmax(t.c_prior[n]) / (t.c_visits[n] + 1).astype(F32)).astype(F32)


def action_scores(t: Tree, n, depth, root_invalid, tb, qtransform=QT_MIN_MAX, min_value=-1.0, max_value=1.0,
                  pb_c_init=1.25, pb_c_base=19652.0):
    """muzero_action_selection's to_argmax (value score + policy score + 1e-7 * tie-break uniform, the root mask at
    depth 0) and the value score's gain d score / d q (near-tie instrumentation)."""
    if qtransform == QT_MIN_MAX:
        vs, gain = qtransform_by_min_max(t, n, min_value, max_value), 1.0 / (float(max_value) - float(min_value))
    elif qtransform == QT_PARENT_SIBLINGS:
        vs, gain = MS.qtransform_by_parent_and_siblings(t, n, with_gain=True)
    else:
        raise ValueError(qtransform)
    score = (vs + puct_policy_score(t, n, pb_c_init, pb_c_base) + F32(1e-7) * np.asarray(tb, F32)).astype(F32)
    if depth == 0:
        score = np.where(root_invalid, -np.inf, score)
    return score, gain


def root_prior_logits(root_logits, invalid, dirichlet, dirichlet_fraction):
    """_add_dirichlet_noise, _get_logits_from_probs, _mask_invalid_actions -> the root's prior logits [B, A]."""
    f = F32(dirichlet_fraction)
    probs = G.softmax(np.asarray(root_logits, F32))
    noisy = ((F32(1.0) - f) * probs + f * np.asarray(dirichlet, F32)).astype(F32)
    logits = log_cr(np.maximum(noisy, F32(TINY)))
    logits = (logits - logits.max(-1, keepdims=True)).astype(F32)
    return np.where(invalid, FMIN, logits).astype(F32)


def final_draw(visits, gumbel, temperature):
    """summary().visit_probs, _apply_temperature, categorical as argmax(logits + Gumbel) for one game ->
    (action, action_weights [A], the argmax's input)."""
    vc = np.asarray(visits).astype(F32)
    w = (vc / max(F32(vc.sum(dtype=F32)), F32(1.0))).astype(F32)
    lw = log_cr(w)
    with np.errstate(over="ignore", invalid="ignore"):
        lw = ((lw - lw.max()) / max(F32(TINY), F32(temperature))).astype(F32)
        x = (lw + np.asarray(gumbel, F32)).astype(F32)
    return int(np.argmax(x)), w, x


def muzero_policy(params, root_logits, root_value, root_embedding, recurrent_fn, num_simulations, invalid_actions,
                  dirichlet, gumbel, max_depth=None, temperature=1.0, qtransform=QT_MIN_MAX, min_value=-1.0,
                  max_value=1.0, dirichlet_fraction=0.25, pb_c_init=1.25, pb_c_base=19652.0, seed=0, turn=0, gids=None,
                  trace=None):
    """mctx.muzero_policy over B games: per-game trees, one batched recurrent_fn(params, action [B], embedding [B, L])
    -> (reward, discount, prior_logits, value, next_embedding) call per simulation.

    Returns (action [B], action_weights [B, A] = root visit fractions, root_value [B] = summary().value, trees).  With
    a dict `trace`, trace['margin'][b] is the smallest normalised top-2 gap (mctx_gumbel.top2_margin) of every argmax
    decision of game b's search (each level of each simulation, and the final draw)."""
    root_logits = np.asarray(root_logits, F32)
    B, A = root_logits.shape
    S = num_simulations
    D = S if max_depth is None else max_depth
    L = root_embedding.shape[1]
    invalid = np.asarray(invalid_actions, bool)
    gids = np.arange(B) if gids is None else np.asarray(gids)
    prior = root_prior_logits(root_logits, invalid, dirichlet, dirichlet_fraction)
    trees = [Tree(S + 1, A, L) for _ in range(B)]
    margins = [[] for _ in range(B)]
    for b, t in enumerate(trees):
        t.update_node(0, prior[b], F32(root_value[b]), root_embedding[b])
    for sim in range(S):
        parents, actions, nexts = [], [], []
        for b, t in enumerate(trees):          # search.py simulate
            node, depth = 0, 0
            while True:
                tb = [MS.tiebreak_uniform(seed, int(gids[b]), turn, sim, depth, a) for a in range(A)]
                score, gain = action_scores(t, node, depth, invalid[b], tb, qtransform, min_value, max_value,
                                            pb_c_init, pb_c_base)
                if trace is not None:
                    margins[b].append(float(G.top2_margin(score[None], gain)[0]))
                a = int(np.argmax(score))
                nxt = int(t.c_index[node, a])
                depth += 1
                if nxt == -1 or depth >= D:
                    break
                node = nxt
            parents.append(node)
            actions.append(a)
            nexts.append(sim + 1 if nxt == -1 else nxt)
        # search.py expand
        r, d, lg, v, ne = recurrent_fn(params, np.array(actions, np.int32),
                                       np.stack([trees[b].emb[parents[b]] for b in range(B)]))
        for b, t in enumerate(trees):
            p, a, nn = parents[b], actions[b], nexts[b]
            t.update_node(nn, np.asarray(lg[b], F32), F32(v[b]), ne[b])
            t.c_index[p, a], t.c_reward[p, a], t.c_disc[p, a] = nn, F32(r[b]), F32(d[b])
            t.parent[nn], t.afp[nn] = p, a
            # search.py backward
            idx = nn
            leaf = F32(t.value[idx])
            while idx != 0:
                p = t.parent[idx]
                cnt = t.visits[p]
                a = t.afp[idx]
                leaf = F32(t.c_reward[p, a] + F32(t.c_disc[p, a] * leaf))
                t.value[p] = F32(F32(F32(t.value[p] * F32(cnt)) + leaf) / (F32(cnt) + F32(1.0)))
                t.visits[p] = cnt + 1
                t.c_value[p, a] = t.value[idx]
                t.c_visits[p, a] += 1
                idx = p
    action = np.zeros(B, np.int32)
    weights = np.zeros((B, A), F32)
    rv = np.zeros(B, F32)
    for b, t in enumerate(trees):
        action[b], weights[b], x = final_draw(t.c_visits[0], gumbel[b], temperature)
        if trace is not None:
            margins[b].append(float(G.top2_margin(x[None])[0]))
        rv[b] = t.value[0]
    if trace is not None:
        trace["margin"] = np.array([min(m) if m else np.inf for m in margins])
    return action, weights, rv, trees
