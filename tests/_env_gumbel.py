"""NumPy restatement of the Gumbel network-free MCTS agent for det-MADN (TEST INFRASTRUCTURE ONLY): mctx
gumbel_muzero_policy whose model is the environment itself, with random-rollout leaf values -- the call the reference
drives (MADN/simulate_deterministicMADN.py:12-35 run_gumbel over root_fn / recurrent_fn of
MADN/deterministic_madn.py:481-589, with qtransform_by_min_max(-1, 1)).

The reference's path cannot run as written (tests/_env_mcts.py says why), and mctx masks the root only.  Parity with
the reference: UNPINNED.  This file is the definition; csrc/env_gumbel.hip equals it bit for bit, one game at a time.

Composed from
  tests/_env_mcts.py      the model: node_mask, wins_fast, transition, rollout, prior_logits, the fixture loaders;
  oracle/mctx_gumbel.py   the search: the considered-visit sequence, score_considered, masked_argmax, softmax,
                          mask_invalid_actions, qtransform_completed_by_mix_value, Tree / update_tree_node (B = 1);
  tests/_mctx_muzero.py   qtransform_by_min_max's arithmetic.
It carries its own simulate loop, because every node is masked the way the root is (as in tests/_env_mcts.py): the
prior logit is FMIN outside the node's mask and the interior score -inf there -- a legal child's softmax - visit share
can be negative, and an illegal unvisited child would score 0 and win.  A node with mask 0 counts as all 24 actions
legal.  No Dirichlet noise, no tie-break uniform; every argmax takes the first maximum.

  root prior   the masked logits 100 legal + 200 wins minus their maximum, FMIN outside the mask
  root score   score_considered(considered visit of (min(max_num_considered, legal count), S, sum of root visits))
  interior     softmax(prior + cq) - N / (1 + sum N), -inf outside the node's mask
  cq           "completed_by_mix_value": qtransform_completed_by_mix_value(value_scale, maxvisit_init), rescaled;
               "min_max": qtransform_by_min_max(min_value, max_value) (the reference's call)
  tail         action: argmax of the root score with considered visit max(visits); weights: softmax(mask(prior + cq));
               value: the root node's value; visits / qvalues: the root's summary; turns: the rollout turns played
  not searched a root that is done or has no legal action: action -1, weights 0, value 0."""
from __future__ import annotations

import numpy as np

from oracle import mctx_gumbel as G
from tests import _env_mcts as EM

F32 = np.float32
A = EM.A
ALL = EM.ALL
QT_COMPLETED_MIX, QT_MIN_MAX = "completed_by_mix_value", "min_max"
ROOT = np.zeros(1, np.int32)


def completed_q(t: G.Tree, node: int, qtransform, value_scale=0.5, maxvisit_init=50.0, min_value=-1.0, max_value=1.0):
    """The qtransform's output for one node of a B = 1 tree -> [A]."""
    n = np.array([node], np.int32)
    if qtransform == QT_COMPLETED_MIX:
        return G.qtransform_completed_by_mix_value(t, n, value_scale=value_scale, maxvisit_init=maxvisit_init)[0]
    if qtransform == QT_MIN_MAX:      # tests/_mctx_muzero.py qtransform_by_min_max on this tree's fields
        q = t.qvalues(n)[0]
        lo, hi = F32(min_value), F32(max_value)
        return ((np.where(t.children_visits[0, node] > 0, q, lo) - lo) / F32(hi - lo)).astype(F32)
    raise ValueError(qtransform)


def interior_scores(t: G.Tree, node: int, mask: int, cq) -> np.ndarray:
    """gumbel_muzero_interior_action_selection's to_argmax with the node's mask: -inf outside it (mask 0: all legal)."""
    visits = t.children_visits[0, node]
    probs = G.softmax((t.children_prior_logits[0, node] + cq).astype(F32)[None])[0]
    score = (probs - visits.astype(F32) / F32(1 + visits.sum())).astype(F32)
    return np.where(EM.bits_to_bool(mask if mask else ALL), score, -np.inf)


def root_scores(t: G.Tree, considered_visit: int, gumbel, cq) -> np.ndarray:
    return G.score_considered(considered_visit, np.asarray(gumbel, F32), t.children_prior_logits[0, 0], cq,
                              t.children_visits[0, 0])


def search_one(env, S, D, rollout_steps, seed, turn, gid, gumbel, qtransform=QT_COMPLETED_MIX, max_num_considered=16,
               value_scale=0.5, maxvisit_init=50.0, min_value=-1.0, max_value=1.0):
    """One game's search -> dict(action, weights, value, visits, qvalues, turns, tree) (tree None when not searched);
    gumbel [A]: the root's (already scaled) Gumbel noise."""
    lm = EM.node_mask(env)
    if lm == 0:
        return dict(action=-1, weights=np.zeros(A, F32), value=F32(0), visits=np.zeros(A, np.int32),
                    qvalues=np.zeros(A, F32), turns=0, tree=None)
    qkw = dict(value_scale=value_scale, maxvisit_init=maxvisit_init, min_value=min_value, max_value=max_value)
    gumbel = np.asarray(gumbel, F32)
    invalid = ~EM.bits_to_bool(lm)
    wm = EM.wins_fast(env, lm)
    logits = (F32(100.0) * EM.bits_to_bool(lm).astype(F32) + F32(200.0) * EM.bits_to_bool(wm).astype(F32)).astype(F32)
    prior = G.mask_invalid_actions(logits[None], invalid[None])[0]
    value, turns = EM.rollout(env, seed, gid, turn, 0, rollout_steps)
    cv_seq = G.get_sequence_of_considered_visits(min(max_num_considered, int((~invalid).sum())), S)
    t = G.Tree(1, S, A, 1)
    G.update_tree_node(t, ROOT, prior[None], np.array([value], F32), np.zeros((1, 1), F32))
    states, masks = [env] + [None] * S, [lm] + [0] * S
    for sim in range(S):
        node, depth = 0, 0
        while True:                                   # search.py simulate, every node masked
            cq = completed_q(t, node, qtransform, **qkw)
            if depth == 0:
                score = root_scores(t, cv_seq[int(t.children_visits[0, 0].sum())], gumbel, cq)
                a = int(G.masked_argmax(score[None], invalid[None])[0])
            else:
                a = int(np.argmax(interior_scores(t, node, masks[node], cq)))
            nxt = int(t.children_index[0, node, a])
            depth += 1
            if nxt == -1 or depth >= D:
                break
            node = nxt
        nn = sim + 1 if nxt == -1 else nxt
        s2, r, d, _ = EM.transition(states[node], a)    # search.py expand: recurrent_fn is the environment
        m2 = EM.node_mask(s2)
        v = F32(0)
        if not s2.done:
            v, n = EM.rollout(s2, seed, gid, turn, sim + 1, rollout_steps)
            turns += n
        nna = np.array([nn], np.int32)
        G.update_tree_node(t, nna, EM.prior_logits(m2, EM.wins_fast(s2, m2) if m2 else 0)[None], np.array([v], F32),
                           np.zeros((1, 1), F32))
        states[nn], masks[nn] = s2, m2
        t.children_index[0, node, a] = nn
        t.children_rewards[0, node, a] = F32(r)
        t.children_discounts[0, node, a] = F32(d)
        t.parents[0, nn], t.action_from_parent[0, nn] = node, a
        G.backward(t, nna)                              # search.py backward
    visits = t.children_visits[0, 0]
    cq = completed_q(t, 0, qtransform, **qkw)
    action = int(G.masked_argmax(root_scores(t, int(visits.max()), gumbel, cq)[None], invalid[None])[0])
    weights = G.softmax(G.mask_invalid_actions((prior + cq).astype(F32)[None], invalid[None]))[0]
    return dict(action=action, weights=weights, value=F32(t.node_values[0, 0]), visits=visits.copy(),
                qvalues=t.qvalues(ROOT)[0], turns=turns, tree=t)


def env_gumbel_muzero_policy(envs, S, D, rollout_steps, seed, turn, gids=None, gumbel=None, **kw):
    """The batch: per-game searches stacked -> dict of arrays (action [B], weights / visits / qvalues [B, 24], value
    [B], turns [B]).  gumbel [B, 24] (zeros when left out: Gumbel scale 0)."""
    B = len(envs)
    gids = np.arange(B) if gids is None else np.asarray(gids)
    gumbel = np.zeros((B, A), F32) if gumbel is None else gumbel
    rs = [search_one(e, S, D, rollout_steps, seed, turn, int(gids[b]), gumbel[b], **kw) for b, e in enumerate(envs)]
    return {k: np.stack([np.asarray(r[k]) for r in rs]) for k in ("action", "weights", "value", "visits", "qvalues",
                                                                  "turns")}
