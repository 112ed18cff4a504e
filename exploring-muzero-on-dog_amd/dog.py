"""Batched DOG environment on the GPU (host mirror of DOG/dog.py).

Same conventions as ``detmadn.py`` / ``classic.py``: one ``DOGState`` holds B games as device-resident
field-major SoA tensors (include/muz.h ``muz_dog_soa``); every call is one HIP launch over the batch and
updates the state in place.  One wavefront owns a game (csrc/env_dog.hip).

Reference entry points mirrored (file:line in the reference):
  env_reset / distribute_cards / reset_deck   DOG/dog.py:83-186, 201-298, 188-191
  valid_actions (-> valid_step_actions)       DOG/dog.py:693-711 (617-691)
  env_step (play / swap phase)                DOG/dog.py:1117-1131 (986-1062, 1077-1114)
  no_step                                     DOG/dog.py:713-752
  map_action_to_move / map_move_to_action     DOG/dog.py:1133-1239 (host helpers below)

The shuffle keys of a deal come from the engine's counter RNG (include/muz.h, DOG section) instead of
jax threefry; ``oracle/dog.py:engine_shuffle_keys`` restates them for the parity tests.  The
reference's ``encode_board`` is a stub (dog.py:1264-1272), so there is no DOG observation here.

``rollout_policy`` is the network-free rollout agent (csrc/dog_rollout.hip): the reference has no DOG agent that
runs, so it is this engine's own and parity-unpinned; ``tests/_dog_rollout.py`` defines it.  ``greedy_policy`` is the
one-ply greedy agent and ``afterstate_features`` the per-action board features it scores (csrc/dog_greedy.hip), the
engine's own in the same way; ``tests/_dog_greedy.py`` defines them.  ``guided_rollout_policy`` is the rollout agent
whose playout turns pick among the greedy agent's best-scored actions (csrc/dog_guided.hip); ``tests/_dog_guided.py``
defines it.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import lib as _L
from . import soa as _S

CELLS = 56
CARDS = 14
ACTIONS = 806
PLAY_ACTIONS = 792
BASE = 396
MASK_WORDS = 26
NORMAL_MOVES = (1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13)

# env_reset keyword defaults (dog.py:83-100)
DEFAULT_RULES = dict(
    enable_teams=False,
    enable_initial_free_pin=False,
    enable_circular_board=True,
    enable_start_blocking=False,
    enable_jump_in_goal_area=True,
    enable_friendly_fire=False,
    must_traverse_start=True,
    disable_swapping=False,
    disable_hot_seven=False,
    disable_joker=False,
)

# MuZero_DOG/game_agent.py:12-23 (config (d))
SELFPLAY_RULES = dict(
    enable_teams=True,
    enable_initial_free_pin=False,
    enable_circular_board=True,
    enable_friendly_fire=True,
    enable_start_blocking=True,
    enable_jump_in_goal_area=False,
    must_traverse_start=True,
    disable_swapping=False,
    disable_hot_seven=False,
    disable_joker=False,
)


def all_pin_distributions(total=7):
    """utils/utility_funcs.py:4-21: lex order over (a0, a1, a2), a3 = total - a0 - a1 - a2 >= 0."""
    return np.array([(a, b, c, total - a - b - c) for a in range(total + 1) for b in range(total + 1)
                     for c in range(total + 1) if total - a - b - c >= 0], np.int32)


DISTS_7_4 = all_pin_distributions(7)


def make_rules(num_players=4, layout=(True, True, True, True), distance=10, starting_player=0, **rules):
    return _S.make_rules(DEFAULT_RULES, num_players, layout, distance, starting_player, **rules)


@dataclass
class DOGState(_S.SoAState):
    """SoA batch state. Field c of game b is ``field[c, b]``."""

    board: torch.Tensor           # int8 [56, B]
    pins: torch.Tensor            # int8 [P*4, B]
    deck: torch.Tensor            # int8 [14, B]
    hands: torch.Tensor           # int8 [P*14, B]
    swap_choices: torch.Tensor    # int8 [4, B]
    current_player: torch.Tensor  # int8 [B]
    round_starter: torch.Tensor   # int8 [B]
    phase: torch.Tensor           # int8 [B]
    hand_size: torch.Tensor       # int8 [B]
    reward: torch.Tensor          # int8 [B]
    done: torch.Tensor            # uint8 [B]
    deal: torch.Tensor            # int32 [B] (uint32 counter)
    rules: _L.MuzRules
    num_players: int
    seed: int = 0

    ROWS = {"board": lambda P: CELLS, "pins": lambda P: P * 4, "deck": lambda P: CARDS, "hands": lambda P: P * CARDS,
            "swap_choices": lambda P: 4}
    VECTORS = ("current_player", "round_starter", "phase", "hand_size", "reward", "done", "deal")
    DTYPES = {"done": torch.uint8, "deal": torch.int32}
    STRUCT = _L.MuzDogSoA

    def hands_bp(self) -> torch.Tensor:
        return self.hands.T.reshape(self.batch, self.num_players, CARDS)


def _call(name, *args):
    _L.check(getattr(_L.load(), name)(*args), name)


def env_reset(batch: int, num_players=4, layout=(True, True, True, True), distance=10, starting_player=0,
              seed=0, device="cuda", **rules) -> DOGState:
    """Batched env_reset (dog.py:83-186): empty board, deck (joker 6, others 8), first deal."""
    r = make_rules(num_players, layout, distance, starting_player, **rules)
    st = DOGState.alloc(batch, int(num_players), r, device, seed=int(seed))
    _call("muz_dog_reset", r, st.soa(), ctypes_u64(seed), batch, _L.stream_ptr())
    return st


def ctypes_u64(x: int) -> int:
    return int(x) & 0xFFFFFFFFFFFFFFFF


def state_from_host(fields: dict, rules: _L.MuzRules, seed=0, device="cuda") -> DOGState:
    """Build a batch from host arrays: pins [B,P,4], board [B,56], deck [B,14], hands [B,P,14],
    swap_choices [B,4], and per-game scalars current_player / round_starter / phase / hand_size / reward /
    done / deal."""
    pins = np.asarray(fields["pins"], np.int8)
    B, P, _ = pins.shape
    st = DOGState.alloc(B, P, rules, device, seed=int(seed))

    def put(dst, a):
        dst.copy_(torch.from_numpy(np.ascontiguousarray(a)))

    put(st.board, np.asarray(fields["board"], np.int8).T)
    put(st.pins, pins.reshape(B, P * 4).T)
    put(st.deck, np.asarray(fields["deck"], np.int8).T)
    put(st.hands, np.asarray(fields["hands"], np.int8).reshape(B, P * CARDS).T)
    put(st.swap_choices, np.asarray(fields["swap_choices"], np.int8).T)
    for k in ("current_player", "round_starter", "phase", "hand_size", "reward"):
        put(getattr(st, k), np.asarray(fields[k], np.int8).reshape(B))
    put(st.done, np.asarray(fields["done"], np.uint8).reshape(B))
    put(st.deal, np.asarray(fields["deal"], np.int64).astype(np.uint32).view(np.int32).reshape(B))
    return st


def to_host(st: DOGState) -> dict:
    """Per-game host view of the batch (inverse of state_from_host)."""
    B, P = st.batch, st.num_players
    return dict(board=st.board.T.cpu().numpy(), pins=st.pins.T.cpu().numpy().reshape(B, P, 4),
                deck=st.deck.T.cpu().numpy(), hands=st.hands.T.cpu().numpy().reshape(B, P, CARDS),
                swap_choices=st.swap_choices.T.cpu().numpy(), current_player=st.current_player.cpu().numpy(),
                round_starter=st.round_starter.cpu().numpy(), phase=st.phase.cpu().numpy(),
                hand_size=st.hand_size.cpu().numpy(), reward=st.reward.cpu().numpy(),
                done=st.done.cpu().numpy(), deal=st.deal.cpu().numpy().view(np.uint32))


def legal_mask(env: DOGState, out: torch.Tensor | None = None) -> torch.Tensor:
    """valid_actions as bitsets int32 [B, 26]."""
    out = torch.empty((env.batch, MASK_WORDS), dtype=torch.int32, device=env.board.device) if out is None else out
    _call("muz_dog_legal", env.rules, env.soa(), _L.ptr(out), env.batch, _L.stream_ptr())
    return out


def unpack_mask(bits: torch.Tensor) -> torch.Tensor:
    sh = torch.arange(32, device=bits.device, dtype=torch.int32)
    return ((bits[:, :, None] >> sh) & 1).reshape(bits.shape[0], MASK_WORDS * 32)[:, :ACTIONS].bool()


def valid_actions(env: DOGState) -> torch.Tensor:
    """valid_actions (dog.py:693-711) -> bool [B, 806]."""
    return unpack_mask(legal_mask(env))


def env_step(env: DOGState, action: torch.Tensor, seed: int | None = None):
    """env_step (dog.py:1117-1131), in place; a negative action applies no_step.  Returns (env, reward, done)."""
    dev = env.board.device
    action = action.to(device=dev, dtype=torch.int32).reshape(env.batch).contiguous()
    reward = torch.empty((env.batch,), dtype=torch.int8, device=dev)
    done = torch.empty((env.batch,), dtype=torch.uint8, device=dev)
    s = env.seed if seed is None else seed
    _call("muz_dog_step", env.rules, env.soa(), _L.ptr(action), ctypes_u64(s), _L.ptr(reward), _L.ptr(done),
          env.batch, _L.stream_ptr())
    return env, reward, done.bool()


def no_step(env: DOGState, seed: int | None = None):
    """no_step (dog.py:713-752), in place.  Returns (env, reward, done)."""
    dev = env.board.device
    reward = torch.empty((env.batch,), dtype=torch.int8, device=dev)
    done = torch.empty((env.batch,), dtype=torch.uint8, device=dev)
    s = env.seed if seed is None else seed
    _call("muz_dog_nostep", env.rules, env.soa(), ctypes_u64(s), _L.ptr(reward), _L.ptr(done), env.batch,
          _L.stream_ptr())
    return env, reward, done.bool()


STEP_KINDS = {"swap": 0, "normal": 1, "neg": 2, "hot7": 3}


def step_move(env: DOGState, kind, args):
    """step_swap / step_normal_move / step_neg_move / step_hot_7 (dog.py:754-984) on their own, one per game:
    kind[b] in STEP_KINDS, args[b] = (pin, pos|move, 0, 0) or the 4-pin distribution.  Board and pins change
    in place; returns (env, reward, done) like the reference functions."""
    dev = env.board.device
    k = torch.as_tensor(np.asarray([STEP_KINDS.get(x, x) for x in kind], np.int32), device=dev)
    a = torch.as_tensor(np.asarray(args, np.int32).reshape(env.batch, 4), device=dev).contiguous()
    reward = torch.empty((env.batch,), dtype=torch.int8, device=dev)
    done = torch.empty((env.batch,), dtype=torch.uint8, device=dev)
    _call("muz_dog_step_move", env.rules, env.soa(), _L.ptr(k), _L.ptr(a), _L.ptr(reward), _L.ptr(done), env.batch,
          _L.stream_ptr())
    return env, reward, done.bool()


def random_action(mask: torch.Tensor, uniform: torch.Tensor | None = None, seed=0, turn=0,
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """Uniform random legal action per game from the bitset mask (-1 if none)."""
    B = mask.shape[0]
    out = torch.empty((B,), dtype=torch.int32, device=mask.device) if out is None else out
    u = None if uniform is None else uniform.to(device=mask.device, dtype=torch.float32).contiguous()
    _call("muz_dog_random_action", _L.ptr(mask), _L.ptr(u), ctypes_u64(seed), int(turn), _L.ptr(out), B,
          _L.stream_ptr())
    return out


# ---- the network-free rollout agent (csrc/dog_rollout.hip; include/muz.h, DOG rollout agent) -------------------------
class RolloutWorkspace:
    """The device workspace of ``rollout_policy`` for up to ``n`` games (muz_dog_rollout_bytes)."""

    def __init__(self, n: int, device="cuda"):
        self.n = int(n)
        self.buf = torch.empty((int(_L.load().muz_dog_rollout_bytes(self.n)),), dtype=torch.uint8, device=device)


def rollout_policy(env, rollouts: int = 4, *, max_phases: int = 10, rollout_steps: int = 300, determinize: bool = True,
                   seed: int, turn: int, game_id: torch.Tensor | None = None,
                   workspace: RolloutWorkspace | None = None, summary: bool = False):
    """The rollout agent's action for every game of ``env`` (int32 [B]; -1 for a finished game or one without a legal
    action): every legal action is tried on copies of the game whose hidden cards are re-drawn (``determinize``), each
    copy is played out with the random policy for at most ``rollout_steps`` turns, and the actions are thinned by
    sequential halving on their win counts, ``rollouts`` playouts per action and phase, at most ``max_phases`` phases
    (muz_dog_rollout_search; the semantics are in include/muz.h, the definition is tests/_dog_rollout.py -- the
    reference has no DOG agent, parity is unpinned).  ``env`` is not changed.  The playouts are keyed by ``seed``,
    ``turn`` and ``game_id`` (default: the position in the batch), so both are required.  With ``summary`` returns
    (action, value float32 [B], visits int32 [B, 806], wins int32 [B, 806], rollout_turns int32 [B])."""
    if not isinstance(env, DOGState):
        raise TypeError(f"rollout_policy searches a DOG state (dog.DOGState), not {type(env).__name__}")
    B, dev = env.batch, env.board.device
    if workspace is None:
        workspace = RolloutWorkspace(B, dev)
    if workspace.n < B:
        raise ValueError(f"the workspace holds {workspace.n} games, the state {B}")
    cfg = _L.MuzDogRolloutCfg(int(rollouts), int(max_phases), int(rollout_steps), int(bool(determinize)),
                              ctypes_u64(seed), int(turn))
    gid = None if game_id is None else game_id.to(device=dev, dtype=torch.int32).reshape(B).contiguous()
    action = torch.empty((B,), dtype=torch.int32, device=dev)
    value = torch.empty((B,), dtype=torch.float32, device=dev)
    visits = wins = turns = None
    if summary:
        visits = torch.empty((B, ACTIONS), dtype=torch.int32, device=dev)
        wins = torch.empty((B, ACTIONS), dtype=torch.int32, device=dev)
        turns = torch.empty((B,), dtype=torch.int32, device=dev)
    _call("muz_dog_rollout_search", env.rules, ctypes.byref(cfg), env.soa(), _L.ptr(gid), _L.ptr(action), _L.ptr(value),
          _L.ptr(visits), _L.ptr(wins), _L.ptr(turns), B, _L.ptr(workspace.buf), _L.nbytes(workspace.buf),
          _L.stream_ptr())
    return (action, value, visits, wins, turns) if summary else action


# ---- the one-ply greedy agent (csrc/dog_greedy.hip; include/muz.h, DOG greedy agent) ---------------------------------
GREEDY_FEATURES = ("advance", "setback", "goal", "out", "hit", "win")
GREEDY_DEFAULTS = dict(advance=1, setback=1, goal=20, out=15, hit=10, win=1000, temperature=0.25)


def _greedy(env, name, w, temperature, seed, turn, game_id, want_scores, want_features):
    if not isinstance(env, DOGState):
        raise TypeError(f"{name} scores the afterstates of a DOG state (dog.DOGState), not {type(env).__name__}")
    B, dev = env.batch, env.board.device
    cfg = _L.MuzDogGreedyCfg((ctypes.c_int32 * 6)(*[int(x) for x in w]), float(temperature), ctypes_u64(seed),
                             int(turn))
    gid = None if game_id is None else game_id.to(device=dev, dtype=torch.int32).reshape(B).contiguous()
    action = torch.empty((B,), dtype=torch.int32, device=dev)
    scores = torch.empty((B, ACTIONS), dtype=torch.int32, device=dev) if want_scores else None
    features = torch.empty((B, ACTIONS, 6), dtype=torch.int32, device=dev) if want_features else None
    _call("muz_dog_greedy_action", env.rules, ctypes.byref(cfg), env.soa(), _L.ptr(gid), _L.ptr(action),
          _L.ptr(scores), _L.ptr(features), B, _L.stream_ptr())
    return action, scores, features


def afterstate_features(env) -> torch.Tensor:
    """The six board features of every legal action's afterstate (int32 [B, 806, 6]: advance, setback, goal, out, hit,
    win; 0 for an illegal action and for the swap phase's card choices): env_step tried once per legal action on the
    real environment, without the deal it may ask for, and the board it leads to compared with the root's (include/muz.h,
    DOG greedy agent; the definition is tests/_dog_greedy.py).  One launch (muz_dog_greedy_action with all weights 0);
    ``env`` is not changed."""
    return _greedy(env, "afterstate_features", (0,) * 6, 0.0, 0, 0, None, False, True)[2]


def greedy_policy(env, *, weights: dict | None = None, temperature: float | None = None, seed: int, turn: int,
                  game_id: torch.Tensor | None = None, summary: bool = False):
    """The one-ply greedy agent's action for every game of ``env`` (int32 [B]; -1 for a finished game or one without a
    legal action): every legal action is tried once on the real environment and scored by the board it leads to,
    score = sum of ``weights`` (a dict over GREEDY_FEATURES; missing keys take GREEDY_DEFAULTS; integers in
    [-32768, 32767]) times ``afterstate_features``; at ``temperature`` 0 the first action with the greatest score, else
    the argmax of score / temperature plus the scripted agents' Gumbel draw, keyed by ``seed``, ``turn`` and
    ``game_id`` (default: the position in the batch), so both are required (muz_dog_greedy_action; the semantics are in
    include/muz.h, the definition is tests/_dog_greedy.py -- the reference has no DOG agent that runs, parity is
    unpinned).  One launch; ``env`` is not changed.  With ``summary`` returns (action, scores int32 [B, 806] --
    INT32_MIN for an illegal action --, features int32 [B, 806, 6])."""
    v = dict(GREEDY_DEFAULTS)
    unknown = set(weights or {}) - set(GREEDY_FEATURES)
    if unknown:
        raise ValueError(f"unknown greedy weights {sorted(unknown)} (the features are {GREEDY_FEATURES})")
    v.update(weights or {})
    t = v["temperature"] if temperature is None else temperature
    action, scores, features = _greedy(env, "greedy_policy", [v[k] for k in GREEDY_FEATURES], t, seed, turn, game_id,
                                       summary, summary)
    return (action, scores, features) if summary else action


# ---- the rollout agent with greedy-guided playouts (csrc/dog_guided.hip; include/muz.h, DOG guided rollout agent) -----
GUIDED_EPSILON = 0.125   # an unmeasured choice, exact in float32 (profiles/dog_guided_bench.log reports other values)


def guided_rollout_policy(env, rollouts: int = 4, *, weights: dict | None = None, epsilon: float = GUIDED_EPSILON,
                          max_phases: int = 10, rollout_steps: int = 300, determinize: bool = True, seed: int,
                          turn: int, game_id: torch.Tensor | None = None, workspace: RolloutWorkspace | None = None,
                          summary: bool = False):
    """``rollout_policy`` with greedy-guided playouts (int32 [B]; -1 for a finished game or one without a legal action):
    the same root-level search -- candidates, phases, sequential halving, re-drawn hidden cards, streams --, but a
    playout turn picks uniformly among the actions the greedy agent scores best (``weights``: a dict over
    GREEDY_FEATURES, missing keys take GREEDY_DEFAULTS, integers in [-32768, 32767]; there is no temperature), and with
    probability ``epsilon`` (a float32 in [0, 1]) uniformly among all legal actions, as the random playout does.  With
    ``epsilon`` 1 it is ``rollout_policy``, output for output (muz_dog_guided_rollout_search; the semantics are in
    include/muz.h, the definition is tests/_dog_guided.py -- the reference has no DOG agent that runs, parity is
    unpinned).  ``env`` is not changed; ``workspace`` is ``rollout_policy``'s.  With ``summary`` returns (action, value
    float32 [B], visits int32 [B, 806], wins int32 [B, 806], rollout_turns int32 [B], decided int32 [B]: the rollouts
    of a game whose outcome was not 0)."""
    if not isinstance(env, DOGState):
        raise TypeError(f"guided_rollout_policy searches a DOG state (dog.DOGState), not {type(env).__name__}")
    unknown = set(weights or {}) - set(GREEDY_FEATURES)
    if "temperature" in unknown:
        raise ValueError("guided_rollout_policy has no temperature: a playout turn picks uniformly among the "
                         "best-scored actions, and epsilon sets the share of uniformly random turns")
    if unknown:
        raise ValueError(f"unknown greedy weights {sorted(unknown)} (the features are {GREEDY_FEATURES})")
    v = dict(GREEDY_DEFAULTS)
    v.update(weights or {})
    eps = float(epsilon)
    if not 0.0 <= eps <= 1.0:
        raise ValueError(f"epsilon is a probability in [0, 1], not {epsilon!r}")
    B, dev = env.batch, env.board.device
    if workspace is None:
        workspace = RolloutWorkspace(B, dev)
    if workspace.n < B:
        raise ValueError(f"the workspace holds {workspace.n} games, the state {B}")
    cfg = _L.MuzDogGuidedCfg(_L.MuzDogRolloutCfg(int(rollouts), int(max_phases), int(rollout_steps),
                                                 int(bool(determinize)), ctypes_u64(seed), int(turn)),
                             (ctypes.c_int32 * 6)(*[int(v[k]) for k in GREEDY_FEATURES]), eps)
    gid = None if game_id is None else game_id.to(device=dev, dtype=torch.int32).reshape(B).contiguous()
    action = torch.empty((B,), dtype=torch.int32, device=dev)
    value = torch.empty((B,), dtype=torch.float32, device=dev)
    visits = wins = turns = decided = None
    if summary:
        visits = torch.empty((B, ACTIONS), dtype=torch.int32, device=dev)
        wins = torch.empty((B, ACTIONS), dtype=torch.int32, device=dev)
        turns = torch.empty((B,), dtype=torch.int32, device=dev)
        decided = torch.empty((B,), dtype=torch.int32, device=dev)
    _call("muz_dog_guided_rollout_search", env.rules, ctypes.byref(cfg), env.soa(), _L.ptr(gid), _L.ptr(action),
          _L.ptr(value), _L.ptr(visits), _L.ptr(wins), _L.ptr(turns), _L.ptr(decided), B, _L.ptr(workspace.buf),
          _L.nbytes(workspace.buf), _L.stream_ptr())
    return (action, value, visits, wins, turns, decided) if summary else action


# ---- action <-> move helpers (dog.py:1133-1262), host side ---------------------------------------------
def map_action_to_move(action: int):
    """-> (kind, pin, value, joker): kind in {"swap", "hot7", "normal", "neg", "swap_card"}; value = swap
    position / distribution row / move / card."""
    a = int(action)
    if a >= PLAY_ACTIONS:
        return "swap_card", -1, a - PLAY_ACTIONS, False
    joker, i = a < BASE, a % BASE
    if i < 224:
        return "swap", i // CELLS, i % CELLS, joker
    if i < 344:
        return "hot7", -1, i - 224, joker
    if i < 392:
        return "normal", (i - 344) // 12, NORMAL_MOVES[(i - 344) % 12], joker
    return "neg", i - 392, -4, joker


def map_move_to_action(kind: str, pin: int, value: int, joker: bool) -> int:
    off = 0 if joker else BASE
    if kind == "swap_card":
        return PLAY_ACTIONS + int(value)
    if kind == "swap":
        return off + int(pin) * CELLS + int(value)
    if kind == "hot7":
        return off + 224 + int(value)
    if kind == "normal":
        return off + 344 + int(pin) * 12 + NORMAL_MOVES.index(int(value))
    return off + 392 + int(pin)


class RandomPlay:
    """Config (d)'s actor: B DOG games advanced by a uniform random legal action per turn, all on device
    (legal mask -> random action -> step; no_step when nothing is legal, as the step kernel does for -1).
    ``turn()`` is one batched env-step.  ``fused=True`` runs the whole turn as one kernel
    (muz_dog_random_turn: the mask stays in registers, finished games are skipped); otherwise three
    launches (legal mask -> random action -> step) that also step finished games, as env_step would."""

    def __init__(self, batch: int, seed=0, num_players=4, fused=True, **rules):
        r = dict(SELFPLAY_RULES)
        r.update(rules)
        self.env = env_reset(batch, num_players=num_players, seed=seed, **r)
        self.seed = int(seed)
        self.fused = bool(fused)
        self.t = 0
        dev = self.env.board.device
        self.mask = torch.empty((batch, MASK_WORDS), dtype=torch.int32, device=dev)
        self.action = torch.empty((batch,), dtype=torch.int32, device=dev)
        self.reward = torch.empty((batch,), dtype=torch.int8, device=dev)
        self.done = torch.empty((batch,), dtype=torch.uint8, device=dev)
        self._soa = self.env.soa()
        self._lib = _L.load()

    def turn(self):
        e, lib, s = self.env, self._lib, _L.stream_ptr()
        if self.fused:
            _L.check(lib.muz_dog_random_turn(e.rules, self._soa, ctypes_u64(self.seed), self.t, _L.ptr(self.action),
                                             _L.ptr(self.reward), _L.ptr(self.done), e.batch, s),
                     "muz_dog_random_turn")
            self.t += 1
            return
        _L.check(lib.muz_dog_legal(e.rules, self._soa, _L.ptr(self.mask), e.batch, s), "muz_dog_legal")
        _L.check(lib.muz_dog_random_action(_L.ptr(self.mask), None, ctypes_u64(self.seed), self.t,
                                           _L.ptr(self.action), e.batch, s), "muz_dog_random_action")
        _L.check(lib.muz_dog_step(e.rules, self._soa, _L.ptr(self.action), ctypes_u64(self.seed),
                                  _L.ptr(self.reward), _L.ptr(self.done), e.batch, s), "muz_dog_step")
        self.t += 1

    def play(self, nturns: int, env_steps: torch.Tensor | None = None, auto_reset: bool = False,
             episodes: torch.Tensor | None = None, record: "DogTrajectory | None" = None):
        """``nturns`` fused turns in ONE launch (muz_dog_random_play: every game stays in LDS for all of
        them).  ``env_steps`` / ``episodes`` (int32 [B]) accumulate turns played / games finished; with
        ``auto_reset`` a finished game restarts in place and keeps playing.  ``record`` (a DogTrajectory)
        receives one row per turn and game (muz_dog_random_play_record)."""
        e = self.env
        if record is None:
            _L.check(self._lib.muz_dog_random_play(e.rules, self._soa, ctypes_u64(self.seed), self.t, int(nturns),
                                                   int(bool(auto_reset)), _L.ptr(env_steps), _L.ptr(episodes),
                                                   e.batch, _L.stream_ptr()), "muz_dog_random_play")
        else:
            if record.batch != e.batch:
                raise ValueError("record batch differs from the actor's")
            _L.check(self._lib.muz_dog_random_play_record(e.rules, self._soa, ctypes_u64(self.seed), self.t,
                                                          int(nturns), int(bool(auto_reset)), _L.ptr(env_steps),
                                                          _L.ptr(episodes), record.struct(), e.batch,
                                                          _L.stream_ptr()), "muz_dog_random_play_record")
        self.t += int(nturns)


# ---- DOG actor trajectories (config (d): actors -> learner over RCCL) -----------------------------------
DOG_TRAJ_FIELDS = (("act", torch.int32), ("player", torch.int32), ("reward", torch.int32), ("legal", torch.int32),
                   ("done", torch.uint8))


class DogTrajectory:
    """Per-turn records of the DOG actor (muz_dog_traj in include/muz.h): [B, T] action (-1 = no_step),
    player who moved, reward, number of legal actions, game-finished flag, and idx [B] rows recorded.  The
    reference's DOG agent is a stub (MuZero_DOG/game_agent.py:52-57), so this record is the engine's own
    (parity-unpinned); transfer.gather_packed moves packed records to a learner rank like det games."""

    def __init__(self, batch: int, max_steps: int, device="cuda"):
        self.batch, self.T = int(batch), int(max_steps)
        self.buf = {k: torch.zeros((self.batch, self.T), dtype=dt, device=device) for k, dt in DOG_TRAJ_FIELDS}
        self.buf["idx"] = torch.zeros((self.batch,), dtype=torch.int32, device=device)

    def struct(self) -> _L.MuzDogTraj:
        t = _L.MuzDogTraj()
        for k, _ in DOG_TRAJ_FIELDS:
            setattr(t, k, self.buf[k].data_ptr())
        t.idx = self.buf["idx"].data_ptr()
        t.max_steps = self.T
        return t

    def reset(self):
        self.buf["idx"].zero_()

    def pack(self) -> dict:
        """Rows [0, idx) of every lane, contiguous per lane in lane order (the packed layout of
        transfer.pack): every field [R] with R = sum(idx), plus idx [B] and row_offset [B] (int64)."""
        idx = self.buf["idx"]
        full = int(idx.sum().item()) == self.batch * self.T      # one host sync
        if full:        # every lane recorded T rows (e.g. auto-reset play): the [B, T] buffers are the packed rows
            out = {k: self.buf[k].reshape(-1).clone() for k, _ in DOG_TRAJ_FIELDS}
            out["row_offset"] = torch.arange(self.batch, dtype=torch.int64, device=idx.device) * self.T
        else:
            keep = torch.arange(self.T, device=idx.device)[None, :] < idx[:, None]
            flat = keep.reshape(-1).nonzero().squeeze(1)
            out = {k: self.buf[k].reshape(-1).index_select(0, flat) for k, _ in DOG_TRAJ_FIELDS}
            out["row_offset"] = torch.cumsum(idx.to(torch.int64), 0) - idx.to(torch.int64)
        out["idx"] = idx.clone()
        return out
