"""Evaluation harness for det-MADN agents (SURVEY §8f "next" 3; MuZero_det_MADN/evaluate_agent.py).

  test_agent_vs_random          evaluate_agent.py:383-472: the agent plays seat 0 (and seat 2, its
                                partner, when teams are on) with a temperature-0 Gumbel search; the other
                                seats play uniformly random legal moves (multiactor_step_with_random_agent_v2,
                                474-646); no-move turns apply no_step; wins are counted at seat 0
                                (manual_get_winner 16-45); at most 2000 turns.
  compare_agents_statistically  648-713: both agents against random opponents, two-proportion z-test.
  evaluate_agent_parallel       253-311 + play_n_games_for_eval_jitted / play_eval_loop_jitted 715-960: four
                                seats, each a MuZero agent (a DeviceNet, or None = randomly initialised
                                params), 'rule_based_agent' or 'random_agent'; batch_size games per starting
                                player; winners and calculate_progress (129-195) per starting player.
  'mcts_agent'                  a seat name beside the scripted ones (det-MADN only): the reference's network-free
                                MCTS agent (MADN/deterministic_madn.py:481-589: muzero_policy over the real
                                environment with random-rollout leaf values), mcts.env_muzero_policy on the seat's
                                gathered sub-batch with the evaluation's S / D, temperature 0 and no root noise.
  'gumbel_mcts_agent'           the same seat under the Gumbel policy (det-MADN only): the call the reference drives
                                (MADN/simulate_deterministicMADN.py:12-35 run_gumbel), mcts.env_gumbel_muzero_policy
                                with the evaluation's S / D and temperature as its Gumbel scale.
  'stochastic_mcts_agent'       the same for classic MADN (classic only): the reference's sketch with chance nodes for
                                the die (MADN/classic_madn.py:543-714), stochastic.env_stochastic_muzero_policy.
  'rollout_agent'               DOG's network-free seat (DOG only): a root-level Monte-Carlo search over the real
                                environment with re-drawn hidden cards, dog.rollout_policy (the reference has no DOG
                                agent that runs; parity unpinned).
  'greedy_agent'                DOG's cheap scripted seat (DOG only): every legal action tried once on the real
                                environment and scored by the board it leads to, dog.greedy_policy over the whole
                                batch (the reference's rule-based DOG agent cannot run; parity unpinned).
  'guided_rollout_agent'        the rollout seat with greedy-guided playouts (DOG only): dog.guided_rollout_policy, whose
                                playout turns pick among the greedy agent's best-scored actions (parity unpinned).
  policy_action                 the random agent (770-775) and the rule-based agent (777-864) as one device
                                kernel (muz_detmadn_policy_action), sampling by Gumbel-max on the counter RNG.

Everything runs batched on the GPU: one legal-mask launch per turn, the agent's games go through
encode -> root inference -> muz_gumbel_search as one sub-batch, the random seats draw from the legal
bitmask on the device, and env_step / no_step run on sub-batches of the SoA state.  Differences from the
reference, on purpose: the starting player cycles over the games (game % P) instead of a jax random draw,
and the random seats use torch's generator (the reference's jax keys are not restated).

The classic-MADN and the DOG harness (MuZero_Classic_MADN/evaluate_agent_stochastic.py, MuZero_DOG/evaluate_agent.py)
run the same four-seat loop (_four_seats around _turn); what differs between the three games is in _Det, _Classic and
_Dog.
"""
from __future__ import annotations

import math

import torch

from . import classic as CL
from . import detmadn as E
from . import dog as DOG
from . import lib as _L
from . import mcts as M
from . import muzero_dog as MD
from . import nets as N
from . import stochastic as ST

# evaluate_agent.py:777-864 (the variant evaluate_agent_parallel runs); 509-603 uses 0.5 / 5 / 3 / 1.5 / 2.5
RULE_AGENT = dict(temperature=0.25, goal_bonus=5.0, out_many=3.0, out_few=2.0, hit_bonus=2.0)

# MuZero_det_MADN/evaluate_agent.py uses the game_agent.py rules
RULES = dict(E.SELFPLAY_RULES)

# the network-free MCTS seat (mcts.env_muzero_policy); rollout cap of MADN/deterministic_madn.py's rollout
MCTS_AGENT = "mcts_agent"
MCTS_ROLLOUT_STEPS = 300
_NO_ENV_MODEL = ("no environment-model search kernel exists for this game (mcts.env_muzero_policy is det-MADN's); use "
                 "'random_agent', 'rule_based_agent' where the game has one, a MuZero agent, or for DOG 'rollout_agent'")
# the same agent under gumbel_muzero_policy (mcts.env_gumbel_muzero_policy), det-MADN's second environment-search seat
GUMBEL_MCTS_AGENT = "gumbel_mcts_agent"
_NO_GUMBEL_CLASSIC = ("the Gumbel environment-model search (mcts.env_gumbel_muzero_policy) is det-MADN's: mctx has no "
                      "Gumbel policy with chance nodes, so classic MADN's network-free seat is "
                      "'stochastic_mcts_agent'; its other named seats are 'rule_based_agent' and 'random_agent'")
_NO_GUMBEL_DOG = ("the Gumbel environment-model search (mcts.env_gumbel_muzero_policy) is det-MADN's: DOG's hidden "
                  "hands have no environment-model search kernel (its network-free seat is 'rollout_agent')")
# classic MADN's network-free MCTS seat (stochastic.env_stochastic_muzero_policy: the same construction with chance
# nodes for the die; rollout cap of MADN/classic_madn.py's rollout, also 300)
STOCHASTIC_MCTS_AGENT = "stochastic_mcts_agent"
_NO_CHANCE_MODEL = ("the environment-model search with chance nodes (stochastic.env_stochastic_muzero_policy) is classic "
                    "MADN's: det-MADN has no die (its seat is 'mcts_agent'), and DOG's hidden hands have no "
                    "environment-model search kernel (its network-free seat is 'rollout_agent')")
# DOG's network-free seat (dog.rollout_policy: root-level Monte-Carlo with re-drawn hidden cards and sequential halving)
ROLLOUT_AGENT = "rollout_agent"
ROLLOUT_DEFAULTS = dict(rollouts=4, rollout_steps=MCTS_ROLLOUT_STEPS, determinize=True)
_NO_ROLLOUT_DET = ("the rollout agent (dog.rollout_policy) is DOG's: det-MADN's network-free seat is 'mcts_agent'; its "
                   "other named seats are 'rule_based_agent' and 'random_agent'")
_NO_ROLLOUT_CLASSIC = ("the rollout agent (dog.rollout_policy) is DOG's: classic MADN's network-free seat is "
                       "'stochastic_mcts_agent'; its other named seats are 'rule_based_agent' and 'random_agent'")
# DOG's scripted seat (dog.greedy_policy: one ply over the real environment, scored on the board); its parameters are
# dog.GREEDY_DEFAULTS
GREEDY_AGENT = "greedy_agent"
_NO_GREEDY_DET = ("the greedy agent (dog.greedy_policy) is DOG's, whose reference rule-based agent cannot run: "
                  "det-MADN's scripted seat is its own 'rule_based_agent'")
_NO_GREEDY_CLASSIC = ("the greedy agent (dog.greedy_policy) is DOG's, whose reference rule-based agent cannot run: "
                      "classic MADN's scripted seat is its own 'rule_based_agent'")
# DOG's rollout seat with greedy-guided playouts (dog.guided_rollout_policy); rollouts, rollout_steps and determinize
# are the rollout seat's, epsilon and the weights come with the evaluation's ``guided`` dict
GUIDED_ROLLOUT_AGENT = "guided_rollout_agent"
_NO_GUIDED_DET = ("the guided rollout agent (dog.guided_rollout_policy) is DOG's: det-MADN's network-free seats are "
                  "'mcts_agent' and 'gumbel_mcts_agent'; its other named seats are 'rule_based_agent' and "
                  "'random_agent'")
_NO_GUIDED_CLASSIC = ("the guided rollout agent (dog.guided_rollout_policy) is DOG's: classic MADN's network-free seat "
                      "is 'stochastic_mcts_agent'; its other named seats are 'rule_based_agent' and 'random_agent'")

# classic MADN, MuZero_Classic_MADN/evaluate_agent_stochastic.py:938-948 (the keys it leaves out take env_reset's
# defaults: no dice rethrow)
CLASSIC_RULES = dict(enable_teams=True, enable_initial_free_pin=True, enable_circular_board=False,
                     enable_friendly_fire=True, enable_start_blocking=False, enable_jump_in_goal_area=True,
                     enable_start_on_1=True, enable_bonus_turn_on_6=True, must_traverse_start=False,
                     enable_dice_rethrow=False)
# do_rule_based of play_eval_loop_jitted (806-866); NUM_SIMULATIONS / MAX_DEPTH / TEMPERATURE of 950-952
CLASSIC_RULE_AGENT = dict(temperature=0.25, goal_bonus=5.0, out_many=3.0, out_few=2.0, hit_bonus=2.5)
CLASSIC_SIMULATIONS, CLASSIC_DEPTH = 75, 50

# DOG, MuZero_DOG/evaluate_agent.py:530-541; NUM_SIMULATIONS / MAX_DEPTH 544-545, TEMPERATURE 0.20 (552: the value the
# script runs with)
DOG_RULES = dict(enable_teams=True, enable_initial_free_pin=False, enable_circular_board=True, enable_friendly_fire=True,
                 enable_start_blocking=True, enable_jump_in_goal_area=False, must_traverse_start=True,
                 disable_swapping=False, disable_hot_seven=False, disable_joker=False)
DOG_SIMULATIONS, DOG_DEPTH, DOG_TEMPERATURE = 100, 50, 0.2


def random_legal(bits: torch.Tensor, gen: torch.Generator) -> torch.Tensor:
    """A uniformly random set bit of each 24-bit legal mask (jax.random.categorical over valid actions)."""
    mask = E.bits_to_mask(bits).reshape(bits.shape[0], -1).float()
    u = torch.rand(mask.shape, generator=gen, device=bits.device)
    return torch.argmax(torch.where(mask > 0, u, torch.full_like(u, -1.0)), dim=1).to(torch.int32)


def winners(env: E.DetMADNState, teams: bool) -> torch.Tensor:
    """manual_get_winner (evaluate_agent.py:16-45) -> bool [B, P]: players whose goal is full, or the
    finished team (and nobody when both or neither team is done)."""
    P = env.num_players
    pins = env.pins_bp().long()
    done_p = (pins >= 40).all(dim=2)                       # a player's pins only enter its own goal cells
    if not (teams and P == 4):
        return done_p
    t0 = done_p[:, 0] & done_p[:, 2]
    t1 = done_p[:, 1] & done_p[:, 3]
    ok = t0 ^ t1
    w = torch.zeros_like(done_p)
    w[:, 0] = w[:, 2] = ok & t0
    w[:, 1] = w[:, 3] = ok & t1
    return w


@torch.no_grad()
def play_vs_random(net: N.DeviceNet | None, num_games: int, num_players: int = 4, num_simulations: int = 50,
                   max_depth: int = 25, seed: int = 42, max_turns: int = 2000, rules: dict | None = None,
                   device="cuda", *, search: str = "gumbel", rollout_steps: int = MCTS_ROLLOUT_STEPS) -> dict:
    """One batch of games, agent at seat 0 (+2 with teams), random elsewhere.  ``net=None`` makes the
    agent random too (the baseline).  ``search="puct"``: the agent searches with mcts.muzero_policy at temperature 0
    without root noise.  ``net="mcts_agent"``: the network-free MCTS agent (mcts.env_muzero_policy with rollouts of
    at most ``rollout_steps`` turns, keyed by the game's index); ``net="gumbel_mcts_agent"``: the same agent under the
    Gumbel policy (mcts.env_gumbel_muzero_policy).  Returns wins at seat 0, per-seat wins and pins in goal."""
    skw = _search_kwargs(search)
    if isinstance(net, str):
        net = _seat(_Det, net, 0, seed, device)
        if net not in (MCTS_AGENT, GUMBEL_MCTS_AGENT):
            raise ValueError(f"play_vs_random: the agent is a network, None, {MCTS_AGENT!r} or {GUMBEL_MCTS_AGENT!r}, "
                             f"not {net!r}")
    r = dict(RULES if rules is None else rules)
    teams = bool(r.get("enable_teams", False)) and num_players == 4
    P = num_players
    env = E.env_reset(num_games, num_players=P, device=device, **r)
    # starting player = game % P: re-run the reset per starting player on the matching games
    for sp in range(1, P):
        idx = torch.arange(sp, num_games, P, device=device)
        if idx.numel():
            sub = E.env_reset(idx.numel(), num_players=P, starting_player=sp, device=device, **r)
            env.put(idx, sub)
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    ws = _workspace(_Det, [net], num_games, num_simulations, device) if net is not None else None
    env_search = _Det.gumbel_env_search if net == GUMBEL_MCTS_AGENT else _Det.env_search
    mws = _mcts_workspace(_Det, [net], num_games, num_simulations, device)
    for turn in range(max_turns):
        active = env.done == 0
        if not bool(active.any()):
            break
        bits = E.legal_bits(env)
        cp = env.current_player.long()
        agent_seat = (cp == 0) | ((cp == 2) & teams)
        has = bits != 0
        act = torch.zeros(num_games, dtype=torch.int32, device=device)
        mover = active & has
        ag = (mover & agent_seat).nonzero().flatten() if net is not None else mover.new_zeros(0, dtype=torch.long)
        rd = (mover & ~agent_seat).nonzero().flatten() if net is not None else mover.nonzero().flatten()
        if ag.numel() and isinstance(net, str):
            act[ag] = env_search(env.take(ag), ag, num_simulations, max_depth, 0.0, seed, turn, mws, rollout_steps)
        elif ag.numel():
            act[ag] = _Det.search(net, env.take(ag), bits[ag], None, num_simulations, max_depth, 0.0, seed, turn, ws,
                                  skw)
        if rd.numel():
            act[rd] = random_legal(bits[rd], gen)
        _Det.advance(env, act, active, mover)
    w = winners(env, teams)
    in_goal = (env.pins_bp().long() >= 40).sum(dim=2).float().mean(dim=0)
    return {"games": num_games, "wins": int(w[:, 0].sum()), "seat_wins": w.sum(dim=0).tolist(),
            "finished": int(env.done.sum()), "pins_in_goal": in_goal.tolist()}


def test_agent_vs_random(net: N.DeviceNet | None, num_games: int, batch_size: int = 1024, seed: int = 42, *,
                         search: str = "gumbel", **kw) -> tuple:
    """evaluate_agent.py:383-472 -> (wins at seat 0, mean pins in goal per seat); ``search``: "gumbel" or "puct"
    (play_vs_random)."""
    wins, prog, done = 0, None, 0
    for b in range(0, num_games, batch_size):
        r = play_vs_random(net, min(batch_size, num_games - b), seed=seed + b, search=search, **kw)
        wins += r["wins"]
        p = torch.tensor(r["pins_in_goal"]) * r["games"]
        prog = p if prog is None else prog + p
        done += r["games"]
    return wins, (prog / max(done, 1)).tolist()


def z_test(wins1: int, wins2: int, n: int) -> dict:
    """The two-proportion z-test of compare_agents_statistically (evaluate_agent.py:680-693)."""
    w1, w2 = wins1 / n, wins2 / n
    se = math.sqrt(w1 * (1 - w1) / n + w2 * (1 - w2) / n)
    if se > 0:
        z = (w1 - w2) / se
        p = 2 * (1 - 0.5 * (1 + math.erf(abs(z) / math.sqrt(2))))
    else:
        z, p = 0.0, 1.0
    return {"winrate1": w1, "winrate2": w2, "z": z, "p": p, "significant": abs(z) > 1.96}


def compare_agents_statistically(net1, net2, num_games: int = 1000, batch_size: int = 1024, seed: int = 42, **kw):
    """evaluate_agent.py:648-713: each agent against random opponents on the same seeds, then z_test."""
    w1, _ = test_agent_vs_random(net1, num_games, batch_size, seed, **kw)
    w2, _ = test_agent_vs_random(net2, num_games, batch_size, seed, **kw)
    return z_test(w1, w2, num_games)


def _seats(rules, P):
    """Seat (start cell / 10) of each player after env_reset's layout fix-up (deterministic_madn.py:70-74)."""
    lay = [bool(rules.layout[i]) for i in range(4)]
    if sum(lay) != P or (all(lay) and P < 4):
        lay = [i < P for i in range(4)]
    return [i for i in range(4) if lay[i]]


def calculate_progress(env: E.DetMADNState, must_traverse_start: bool = False) -> torch.Tensor:
    """calculate_progress (evaluate_agent.py:129-195) for every game and player -> float32 [B, P]: pins rotated
    to the player's view (home -> pin - 5, track -> (pin - (40 // P) * p) % 40 - traverse, goal -> 40 + offset),
    sorted, and greedily matched to the goal cells 40..43 (repeated masked argmin of |pin - goal|, first index
    on ties).  Note the reference's distance = board_size // num_players (20 at two players, as written)."""
    P = env.num_players
    pins = env.pins_bp().long()                                           # [B, P, 4]
    seats = torch.tensor(_seats(env.rules, P), device=pins.device)
    p_idx = torch.arange(P, device=pins.device)[None, :, None]
    g0 = (40 + 4 * seats)[None, :, None]
    rot = torch.where(pins < 0, pins - 5,
                      torch.where(pins < 40, torch.remainder(pins - (40 // P) * p_idx, 40) - int(must_traverse_start),
                                  40 + (pins - g0)))
    sp = torch.sort(rot, dim=2).values
    dmat = (sp[..., :, None] - (40 + torch.arange(4, device=pins.device))).abs().double()   # [B, P, 4, 4]
    mask = torch.ones_like(dmat, dtype=torch.bool)
    total = torch.zeros(dmat.shape[:2], dtype=torch.float64, device=pins.device)
    inf = torch.full_like(dmat, float("inf"))
    for _ in range(4):
        flat = torch.where(mask, dmat, inf).flatten(2).argmin(dim=2)     # first minimum
        r, c = flat // 4, flat % 4
        total += dmat.flatten(2).gather(2, flat[..., None])[..., 0]
        rows = torch.arange(4, device=pins.device)
        mask &= ~(rows[None, None, :, None] == r[..., None, None])
        mask &= ~(rows[None, None, None, :] == c[..., None, None])
    return total.float()


# ---- the scripted seats ------------------------------------------------------------------------------------------
def _search_kwargs(search: str) -> dict:
    """muzero_mcts keywords of an evaluation seat's search: today's Gumbel call, or the PUCT muzero_policy without
    root noise (the classical MuZero evaluation agent at temperature 0)."""
    if search == "gumbel":
        return {}
    if search == "puct":
        return {"policy": "puct", "dirichlet_fraction": 0.0}
    raise ValueError(f"unknown search {search!r} ('gumbel' or 'puct')")


def _policy_action(entry: str, defaults: dict, env, legal, mode, seed, turn, agent, game_id) -> torch.Tensor:
    m = {"random_agent": 0, "rule_based_agent": 1}[mode]
    a = dict(defaults if agent is None else agent)
    ag = _L.MuzRuleAgent(a["temperature"], a["goal_bonus"], a["out_many"], a["out_few"], a["hit_bonus"])
    out = torch.empty((env.batch,), dtype=torch.int32, device=env.board.device)
    gid = None if game_id is None else game_id.to(device=out.device, dtype=torch.int32).contiguous()
    _L.check(getattr(_L.load(), entry)(env.rules, env.soa(), _L.ptr(legal.contiguous()), m, ag,
                                       int(seed) & ((1 << 64) - 1), int(turn), _L.ptr(gid), _L.ptr(out), env.batch,
                                       _L.stream_ptr()), entry)
    return out


def policy_action(env: E.DetMADNState, legal: torch.Tensor, mode: str, seed: int, turn: int, agent: dict | None = None,
                  game_id: torch.Tensor | None = None) -> torch.Tensor:
    """The random ('random_agent') or rule-based ('rule_based_agent') action of every game (int32 [B], -1
    without a legal action), one launch over the batch (muz_detmadn_policy_action)."""
    return _policy_action("muz_detmadn_policy_action", RULE_AGENT, env, legal, mode, seed, turn, agent, game_id)


def classic_policy_action(env, legal: torch.Tensor, mode: str, seed: int, turn: int, agent: dict | None = None,
                          game_id: torch.Tensor | None = None) -> torch.Tensor:
    """The classic random ('random_agent', do_random 800-804) or rule-based ('rule_based_agent', do_rule_based
    806-866) pin of every game for the die in the state (int32 [B], -1 without a legal pin), one launch
    (muz_classic_policy_action)."""
    return _policy_action("muz_classic_policy_action", CLASSIC_RULE_AGENT, env, legal, mode, seed, turn, agent,
                          game_id)


# ---- what differs between the games ------------------------------------------------------------------------------
def _stepped(env, idx: torch.Tensor, step):
    """``step`` (in place on a state) applied to the games ``idx`` of ``env``."""
    if idx.numel():
        sub = env.take(idx)
        step(sub)
        env.put(idx, sub)


class _Game:
    """What an evaluation turn needs to know about a game: _Det, _Classic and _Dog fill it in (namespaces, never
    instantiated).  ``env`` is the game's environment module, ``RULES`` its evaluation rules; ``search`` returns the
    actions of a gathered sub-batch, ``scripted`` those of the whole batch."""
    REFUSED = {MCTS_AGENT: _NO_ENV_MODEL}      # named agents the game cannot play -> why
    ENV_SEAT = None                            # the name of the game's environment-search seat, if it has one
    GUMBEL_SEAT = None                         # the name of that seat under the Gumbel policy, if the game has one
    ROLLOUT_SEAT = None                        # the name of the game's root-level rollout seat, if it has one
    GREEDY_SEAT = None                         # the name of the game's one-ply greedy scripted seat, if it has one
    GUIDED_SEAT = None                         # the name of the game's guided rollout seat, if it has one

    @classmethod
    def reset(cls, n, sp, seed, device, r):
        return cls.env.env_reset(n, num_players=4, starting_player=sp, device=device, **r)

    @staticmethod
    def pre_turn(env, gen):
        pass

    @classmethod
    def legal(cls, env):
        return cls.env.legal_bits(env)

    @classmethod
    def advance(cls, env, act, active, mover):
        """env_step on the games that move, no_step on the unfinished ones without a legal action."""
        step = mover.nonzero().flatten()
        _stepped(env, step, lambda sub: cls.env.env_step(sub, act[step]))
        _stepped(env, (active & ~mover).nonzero().flatten(), cls.env.no_step)


class _Det(_Game):
    env, RULES, C = E, RULES, E.num_channels(4)
    REFUSED = {STOCHASTIC_MCTS_AGENT: _NO_CHANCE_MODEL, ROLLOUT_AGENT: _NO_ROLLOUT_DET, GREEDY_AGENT: _NO_GREEDY_DET,
               GUIDED_ROLLOUT_AGENT: _NO_GUIDED_DET}
    ENV_SEAT = MCTS_AGENT
    GUMBEL_SEAT = GUMBEL_MCTS_AGENT
    workspace = staticmethod(M.SearchWorkspace)
    env_workspace = staticmethod(M.EnvSearchWorkspace)
    scripted = staticmethod(policy_action)

    @staticmethod
    def has(bits):
        return bits != 0

    @staticmethod
    def random_net(seed, device):
        return N.DeviceNet(N.init_muzero_params(seed, _Det.C), _Det.C, device=device)

    @staticmethod
    def as_net(a, device):
        return N.as_device_net(a, _Det.C, device=device)

    @staticmethod
    def search(net, sub, bits, gid, S, D, temperature, seed, turn, ws, skw):
        out, _ = M.muzero_mcts(net, E.encode_board(sub), bits, S, D, temperature, seed=seed, turn=turn, workspace=ws,
                               **skw)
        return out.action

    @staticmethod
    def env_search(sub, gid, S, D, temperature, seed, turn, mws, rollout_steps=MCTS_ROLLOUT_STEPS):
        """The 'mcts_agent' seat: muzero_policy over the real environment, no root noise, keyed by the games' ids."""
        out, _ = M.env_muzero_policy(sub, S, D, temperature, rollout_steps=rollout_steps, seed=seed, turn=turn,
                                     game_id=gid, workspace=mws)
        return out.action

    @staticmethod
    def gumbel_env_search(sub, gid, S, D, temperature, seed, turn, mws, rollout_steps=MCTS_ROLLOUT_STEPS):
        """The 'gumbel_mcts_agent' seat: gumbel_muzero_policy over the real environment, ``temperature`` its Gumbel
        scale, keyed by the games' ids."""
        out, _ = M.env_gumbel_muzero_policy(sub, S, D, temperature, rollout_steps=rollout_steps, seed=seed, turn=turn,
                                            game_id=gid, workspace=mws)
        return out.action


class _Classic(_Game):
    """play_eval_loop_jitted's body_fn (evaluate_agent_stochastic.py:754-900): throw_die (its dice_probabilities,
    soft lock aware) before the agents move."""
    env, RULES, C = CL, CLASSIC_RULES, CL.num_channels(4)
    REFUSED = {MCTS_AGENT: _NO_ENV_MODEL, ROLLOUT_AGENT: _NO_ROLLOUT_CLASSIC, GUMBEL_MCTS_AGENT: _NO_GUMBEL_CLASSIC,
               GREEDY_AGENT: _NO_GREEDY_CLASSIC, GUIDED_ROLLOUT_AGENT: _NO_GUIDED_CLASSIC}
    ENV_SEAT = STOCHASTIC_MCTS_AGENT
    scripted = staticmethod(classic_policy_action)
    env_workspace = staticmethod(ST.ClassicEnvSearchWorkspace)

    @staticmethod
    def pre_turn(env, gen):
        # the uniform draws of the die: torch's generator (the reference's jax key is not restated)
        CL.throw_die(env, torch.rand((env.batch,), generator=gen, device=env.board.device))

    @staticmethod
    def has(bits):
        return (bits & 15) != 0

    @staticmethod
    def random_net(seed, device):     # a Stochastic MuZero agent with randomly initialised params
        return ST.DeviceClassicNet(ST.init_classic_params(_Classic.C, seed=seed), _Classic.C, device=device)

    @staticmethod
    def as_net(a, device):
        return ST.as_device_classic_net(a, _Classic.C, device=device)

    @staticmethod
    def workspace(n, S, device):
        return torch.empty((_L.load().muz_stochastic_workspace_bytes(n, S),), dtype=torch.uint8, device=device)

    @staticmethod
    def search(net, sub, bits, gid, S, D, temperature, seed, turn, ws, skw):
        return ST.stochastic_muzero_mcts(net, CL.encode_board(sub), bits, S, D, temperature, seed=seed, turn=turn,
                                         game_id=gid, workspace=ws)[0]

    @staticmethod
    def env_search(sub, gid, S, D, temperature, seed, turn, mws, rollout_steps=MCTS_ROLLOUT_STEPS):
        """The 'stochastic_mcts_agent' seat: stochastic_muzero_policy over the real environment (the die of the turn
        is thrown: pre_turn), no root noise, keyed by the games' ids."""
        out, _ = ST.env_stochastic_muzero_policy(sub, S, D, temperature, rollout_steps=rollout_steps, seed=seed,
                                                 turn=turn, game_id=gid, workspace=mws)
        return out.action


class _Dog(_Game):
    """Every game steps in its own lane each turn (a lane that does not move, a finished game's included, applies
    no_step, which leaves a finished game's pins alone), so a game's deals are keyed by its own index."""
    env, RULES = DOG, DOG_RULES
    # do_rule_based (evaluate_agent.py:403-480) is det-MADN's agent copied: valid_mask.reshape(4, 6) of the
    # 806-action DOG mask cannot run, so the reference has no DOG rule-based agent to restate
    REFUSED = {"rule_based_agent": "MuZero_DOG/evaluate_agent.py's rule-based agent reshapes the 806-action mask to "
                                   "(4, 6) and cannot run; use 'random_agent' or a MuZero agent",
               MCTS_AGENT: _NO_ENV_MODEL, STOCHASTIC_MCTS_AGENT: _NO_CHANCE_MODEL, GUMBEL_MCTS_AGENT: _NO_GUMBEL_DOG}
    ROLLOUT_SEAT = ROLLOUT_AGENT
    GREEDY_SEAT = GREEDY_AGENT
    GUIDED_SEAT = GUIDED_ROLLOUT_AGENT
    legal = staticmethod(DOG.legal_mask)
    workspace = staticmethod(MD.SearchWorkspace)
    rollout_workspace = staticmethod(DOG.RolloutWorkspace)

    @staticmethod
    def rollout_search(sub, gid, seed, turn, rws, rollout):
        """The 'rollout_agent' seat: dog.rollout_policy on the seat's gathered games, keyed by the games' ids."""
        return DOG.rollout_policy(sub, seed=seed, turn=turn, game_id=gid, workspace=rws, **rollout)

    @staticmethod
    def guided_search(sub, gid, seed, turn, rws, rollout, guided):
        """The 'guided_rollout_agent' seat: dog.guided_rollout_policy on the seat's gathered games with the rollout
        seat's keywords and workspace and the parameters ``guided`` (epsilon, weights; None: the defaults), keyed by
        the games' ids."""
        return DOG.guided_rollout_policy(sub, seed=seed, turn=turn, game_id=gid, workspace=rws, **rollout,
                                         **(guided or {}))

    @staticmethod
    def reset(n, sp, seed, device, r):   # block sp's deals are keyed by seed + sp
        return DOG.env_reset(n, num_players=4, starting_player=sp, seed=seed + sp, device=device, **r)

    @staticmethod
    def has(legal):
        return (legal != 0).any(dim=1)

    @staticmethod
    def random_net(seed, device):     # the DOG slice's networks, randomly initialised
        return MD.DeviceDogNet(MD.init_muzero_params(seed), device=device)

    @staticmethod
    def as_net(a, device):
        return MD.as_device_net(a, device=device)

    @staticmethod
    def scripted(env, legal, mode, seed, turn, agent, gid):
        """'random_agent', or the 'greedy_agent' seat: dog.greedy_policy over the whole batch with the parameters
        ``agent`` (a dict over dog.GREEDY_DEFAULTS' keys; None: the defaults), keyed by the games' ids."""
        if mode == GREEDY_AGENT:
            a = dict(agent or {})
            temperature = a.pop("temperature", None)
            return DOG.greedy_policy(env, weights=a, temperature=temperature, seed=seed, turn=turn, game_id=gid)
        return DOG.random_action(legal, seed=seed, turn=turn)

    @staticmethod
    def search(net, sub, legal, gid, S, D, temperature, seed, turn, ws, skw):
        lg, v, e = MD.root_inference_fn(net, MD.encode_board(sub), scratch=ws.scratch)
        pol, _ = MD.gumbel_muzero_policy(net, lg, v, e, legal, S, D, temperature, seed=seed, turn=turn, workspace=ws)
        return pol.action

    @staticmethod
    def advance(env, act, active, mover):
        DOG.env_step(env, act)   # -1: no_step (a game without a legal action, or a finished one)


# ---- four seats: evaluate_agent_parallel (evaluate_agent.py:253-311, 715-960) ----------------------------
def _seat(game, a, i, seed, device):
    """Seat i of an evaluation: None -> the game's MuZero agent with randomly initialised params, the name of a
    scripted agent, or anything the game's as_device_*net takes."""
    if a is None:
        return game.random_net(1_000_003 * (seed + 1) + i, device)
    if isinstance(a, str):
        if a in game.REFUSED:
            raise ValueError(game.REFUSED[a])
        if a not in ("rule_based_agent", "random_agent", game.ENV_SEAT, game.GUMBEL_SEAT, game.ROLLOUT_SEAT,
                     game.GREEDY_SEAT, game.GUIDED_SEAT):
            raise ValueError(f"unknown agent {a!r}")
        return a
    return game.as_net(a, device)


def _turn(game, env, seats, gid, turn, seed, gen, S, D, temperature, rule_agent, ws, skw, mws=None,
          rollout_steps=MCTS_ROLLOUT_STEPS, rws=None, rollout=None, guided=None) -> bool:
    """One turn of every unfinished game: per game the agent of its current player -- a search on the gathered
    sub-batch of a seat (a network's, the game's environment-search seat's over the environment -- PUCT or, for the
    game's Gumbel seat, the Gumbel policy --, or the game's rollout seat's with the keywords ``rollout``, its guided
    rollout seat's with ``guided`` besides), or a scripted agent's launch over the batch -- then the game's
    advance.  False, and nothing played, once every game is
    finished."""
    active = env.done == 0
    game.pre_turn(env, gen)
    if not bool(active.any()):
        return False
    legal = game.legal(env)
    cp = env.current_player.long()
    mover = active & game.has(legal)
    act = torch.full((env.batch,), -1, dtype=torch.int32, device=env.board.device)
    for s, a in enumerate(seats):
        sel = mover & (cp == s)
        if not bool(sel.any()):
            continue
        if isinstance(a, str) and a == game.ENV_SEAT:
            idx = sel.nonzero().flatten()
            act[idx] = game.env_search(env.take(idx), gid[idx], S, D, temperature, seed, turn, mws, rollout_steps)
        elif isinstance(a, str) and a == game.GUMBEL_SEAT:
            idx = sel.nonzero().flatten()
            act[idx] = game.gumbel_env_search(env.take(idx), gid[idx], S, D, temperature, seed, turn, mws,
                                              rollout_steps)
        elif isinstance(a, str) and a == game.ROLLOUT_SEAT:
            idx = sel.nonzero().flatten()
            act[idx] = game.rollout_search(env.take(idx), gid[idx], seed, turn, rws,
                                           ROLLOUT_DEFAULTS if rollout is None else rollout)
        elif isinstance(a, str) and a == game.GUIDED_SEAT:
            idx = sel.nonzero().flatten()
            act[idx] = game.guided_search(env.take(idx), gid[idx], seed, turn, rws,
                                          ROLLOUT_DEFAULTS if rollout is None else rollout, guided)
        elif isinstance(a, str):
            act = torch.where(sel, game.scripted(env, legal, a, seed, turn, rule_agent, gid), act)
        else:
            idx = sel.nonzero().flatten()
            act[idx] = game.search(a, env.take(idx), legal[idx], gid[idx], S, D, temperature, seed, turn, ws, skw)
    game.advance(env, act, active, mover)
    return True


def _workspace(game, seats, n, S, device):
    return game.workspace(n, S, device) if any(not isinstance(x, str) for x in seats) else None


def _mcts_workspace(game, seats, n, S, device):
    """The workspace of the game's environment-search seats (one carve serves the PUCT and the Gumbel seat), when one
    of the seats is such an agent."""
    names = [x for x in (game.ENV_SEAT, game.GUMBEL_SEAT) if x is not None]
    if not any(isinstance(x, str) and x in names for x in seats):
        return None
    return game.env_workspace(n, S, device)


def _rollout_workspace(game, seats, n, device):
    """The workspace of the game's rollout seats (one carve serves the rollout and the guided rollout seat), when one of
    the seats is such an agent."""
    names = [x for x in (game.ROLLOUT_SEAT, game.GUIDED_SEAT) if x is not None]
    if not any(isinstance(x, str) and x in names for x in seats):
        return None
    return game.rollout_workspace(n, device)


def _four_seats(game, agents, batch_size, S, D, temperature, seed, rules, max_turns, rule_agent, device, skw,
                report_turns=False, rollout=None, guided=None) -> dict:
    """4 x batch_size games of ``game``, block i started by player i, played to the end or ``max_turns``; the result
    tables, with ``report_turns`` also the number of turns the loop ran."""
    r = dict(game.RULES if rules is None else rules)
    seats = [_seat(game, a, i, seed, device) for i, a in enumerate(agents)]
    n = 4 * batch_size
    env = game.reset(n, 0, seed, device, r)
    for sp in range(1, 4):
        env.put(slice(sp * batch_size, (sp + 1) * batch_size), game.reset(batch_size, sp, seed, device, r))
    gid = torch.arange(n, device=device, dtype=torch.int32)
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    ws = _workspace(game, seats, n, S, device)
    mws = _mcts_workspace(game, seats, n, S, device)
    rws = _rollout_workspace(game, seats, n, device)
    turns = 0
    for turn in range(max_turns):
        turns = turn + 1
        if not _turn(game, env, seats, gid, turn, seed, gen, S, D, temperature, rule_agent, ws, skw, mws, rws=rws,
                     rollout=rollout, guided=guided):
            break
    return _tables(env, r, batch_size, **({"turns": turns} if report_turns else {}))


def _tables(env, r, batch_size, **extra) -> dict:
    """winners[start][player] and average_progress[start][player] as the reference prints them, plus their totals
    (wins per player, progress per player = column sum / 4)."""
    P = env.num_players
    w = winners(env, bool(r.get("enable_teams", False))) & (env.done != 0)[:, None]
    prog = calculate_progress(env, bool(r.get("must_traverse_start", False)))
    win_tab = w.long().reshape(4, batch_size, P).sum(dim=1)
    prog_tab = prog.reshape(4, batch_size, P).mean(dim=1)
    return {"games": env.batch, "winners": win_tab.tolist(), "average_progress": prog_tab.tolist(),
            "wins_per_player": win_tab.sum(dim=0).tolist(), "progress_per_player": (prog_tab.sum(dim=0) / 4).tolist(),
            "finished": int((env.done != 0).sum()), **extra, "final_state": env}


@torch.no_grad()
def evaluate_agent_parallel(agents, batch_size: int = 20, num_simulations: int = 100, max_depth: int = 50,
                            temperature: float = 0.0, seed: int = 0, rules: dict | None = None, max_turns: int = 2000,
                            rule_agent: dict | None = None, device="cuda", *, search: str = "gumbel") -> dict:
    """evaluate_agent_parallel (evaluate_agent.py:253-311): `agents` = the four seats (player indices 0-3),
    each a DeviceNet, None (a MuZero agent with randomly initialised params), 'rule_based_agent',
    'random_agent', 'mcts_agent' (the network-free MCTS over the environment, mcts.env_muzero_policy with S / D,
    temperature and no root noise) or 'gumbel_mcts_agent' (the same agent under the Gumbel policy,
    mcts.env_gumbel_muzero_policy with S / D and temperature as its Gumbel scale).  4 x batch_size games, block i started by player i
    (jnp.repeat(arange(4), batch_size)), at most 2000 turns; MuZero seats search with S / D / temperature (evaluate_agent.py:938-940 defaults) -- the
    Gumbel search, or with ``search="puct"`` mcts.muzero_policy without root noise.
    Returns winners[start][player] and average_progress[start][player] as the reference prints them, plus
    their totals (wins per player, progress per player = column sum / 4)."""
    return _four_seats(_Det, agents, batch_size, num_simulations, max_depth, temperature, seed, rules, max_turns,
                       rule_agent, device, _search_kwargs(search))


# ---- classic MADN: MuZero_Classic_MADN/evaluate_agent_stochastic.py ------------------------------------------------
@torch.no_grad()
def evaluate_agent_parallel_classic(agents, batch_size: int = 150, num_simulations: int = CLASSIC_SIMULATIONS,
                                    max_depth: int = CLASSIC_DEPTH, temperature: float = 0.0, seed: int = 0,
                                    rules: dict | None = None, max_turns: int = 2000, rule_agent: dict | None = None,
                                    device="cuda") -> dict:
    """evaluate_agent_parallel (evaluate_agent_stochastic.py:253-315) with play_n_games_for_eval_jitted /
    play_eval_loop_jitted (717-936): `agents` = the four seats, each a DeviceClassicNet / Flax params (Stochastic
    MuZero, temperature 0, S 75, D 50), None (randomly initialised params), 'rule_based_agent', 'random_agent' or
    'stochastic_mcts_agent' (the network-free MCTS over the dice environment, stochastic.env_stochastic_muzero_policy
    with S / D, temperature and no root noise); 4 x batch_size games, block i started by player i; the die thrown every turn; at most 2000 turns.  Returns
    winners[start][player] and average_progress[start][player] as the reference prints them, and their totals."""
    return _four_seats(_Classic, agents, batch_size, num_simulations, max_depth, temperature, seed, rules, max_turns,
                       rule_agent, device, {})


@torch.no_grad()
def play_vs_random_classic(agent, num_games: int, num_simulations: int = CLASSIC_SIMULATIONS,
                           max_depth: int = CLASSIC_DEPTH, seed: int = 42, max_turns: int = 2000,
                           rules: dict | None = None, device="cuda", *,
                           rollout_steps: int = MCTS_ROLLOUT_STEPS) -> dict:
    """One batch of test_agent_vs_random (evaluate_agent_stochastic.py:387-476): the agent at seat 0 (+ seat 2, its
    partner, with teams) -- a Stochastic MuZero searching at temperature 0 (multiactor_step_with_random_agent_v2,
    478-650), 'rule_based_agent' / 'random_agent', or 'stochastic_mcts_agent' (the network-free MCTS with rollouts of
    at most ``rollout_steps`` turns) -- the other seats random; a random starting player per game
    (env_reset's seed); wins counted at seat 0.  The die is thrown every turn as play_eval_loop_jitted does: the v2
    step as written never throws it, so its games keep env_reset's die 0, have no legal pin and end only at
    MAX_STEPS (oracle/classic_madn.py: valid_action of a fresh state with die 0 is all False)."""
    r = dict(CLASSIC_RULES if rules is None else rules)
    P = 4
    teams = bool(r.get("enable_teams", False))
    ag = _seat(_Classic, agent, 0, seed, device)
    seats = [ag, "random_agent", ag if teams else "random_agent", "random_agent"]
    g = torch.Generator().manual_seed(seed)
    seeds = torch.randint(0, 1_000_000, (num_games,), generator=g).tolist()
    env = CL.env_reset(num_games, num_players=P, starting_player=-1, device=device, seeds=seeds, **r)
    env.rules = CL.make_rules(P, starting_player=0, **r)   # (the seat is in the state now; the kernels take 0..P-1)
    gid = torch.arange(num_games, device=device, dtype=torch.int32)
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    ws = _workspace(_Classic, seats, num_games, num_simulations, device)
    mws = _mcts_workspace(_Classic, seats, num_games, num_simulations, device)
    for turn in range(max_turns):
        if not _turn(_Classic, env, seats, gid, turn, seed, gen, num_simulations, max_depth, 0.0, None, ws, {}, mws,
                     rollout_steps):
            break
    w = winners(env, teams) & (env.done != 0)[:, None]
    prog = calculate_progress(env, bool(r.get("must_traverse_start", False)))
    return {"games": num_games, "wins": int(w[:, 0].sum()), "seat_wins": w.sum(dim=0).tolist(),
            "finished": int((env.done != 0).sum()), "progress": prog.mean(dim=0).tolist()}


def test_agent_vs_random_classic(agent, num_games: int, batch_size: int = 100, seed: int = 42, **kw) -> tuple:
    """test_agent_vs_random (evaluate_agent_stochastic.py:387-476) -> (wins at seat 0, mean final pin distance per
    seat over the batches)."""
    wins, prog, nb = 0, None, 0
    for b in range(0, num_games, batch_size):
        r = play_vs_random_classic(agent, min(batch_size, num_games - b), seed=seed + b, **kw)
        wins += r["wins"]
        p = torch.tensor(r["progress"])
        prog = p if prog is None else prog + p
        nb += 1
    return wins, (prog / max(nb, 1)).tolist()


def compare_agents_statistically_classic(agent1, agent2, num_games: int = 1000, batch_size: int = 100,
                                         seed: int = 42, **kw) -> dict:
    """compare_agents_statistically (evaluate_agent_stochastic.py:652-717): both agents against random opponents on
    the same seeds, then the two-proportion z-test."""
    w1, _ = test_agent_vs_random_classic(agent1, num_games, batch_size, seed, **kw)
    w2, _ = test_agent_vs_random_classic(agent2, num_games, batch_size, seed, **kw)
    return z_test(w1, w2, num_games)


# ---- DOG: MuZero_DOG/evaluate_agent.py --------------------------------------------------------------------------
def _guided_kwargs(guided):
    """The ``guided`` dict of evaluate_agent_parallel_dog: ``epsilon`` and / or ``weights``, nothing else."""
    unknown = set(guided or {}) - {"epsilon", "weights"}
    if unknown:
        raise ValueError(f"unknown guided rollout parameters {sorted(unknown)} (they are 'epsilon' and 'weights'; "
                         "rollouts, rollout_steps and determinize are the evaluation's own keywords)")
    return dict(guided or {})


@torch.no_grad()
def evaluate_agent_parallel_dog(agents, batch_size: int = 20, num_simulations: int = DOG_SIMULATIONS,
                                max_depth: int = DOG_DEPTH, temperature: float = DOG_TEMPERATURE, seed: int = 0,
                                rules: dict | None = None, max_turns: int = 2000, device="cuda", *, rollouts: int = 4,
                                rollout_steps: int = MCTS_ROLLOUT_STEPS, determinize: bool = True,
                                greedy: dict | None = None, guided: dict | None = None) -> dict:
    """evaluate_agent_parallel (MuZero_DOG/evaluate_agent.py:255-313) with play_n_games_for_eval_jitted /
    play_eval_loop_jitted (315-527): `agents` = the four seats, each the DOG slice's MuZero (a DeviceDogNet or its
    flat params; None = randomly initialised params; run_muzero_mcts at A = 806, S 100, D 50, temperature 0.2),
    'random_agent' (do_random: a uniform legal action), 'greedy_agent' (dog.greedy_policy: every legal action tried once
    on the real environment and scored by the board it leads to, with the weights and temperature of ``greedy``, a dict
    over dog.GREEDY_DEFAULTS' keys -- None: the defaults; keyed by seed, turn and the game's index) or
    'rollout_agent' (the network-free root-level Monte-Carlo
    search dog.rollout_policy with ``rollouts`` playouts per action and phase of at most ``rollout_steps`` turns, the
    hidden cards re-drawn when ``determinize``; keyed by seed, turn and the game's index) or 'guided_rollout_agent' (the
    same search with greedy-guided playouts, dog.guided_rollout_policy: ``rollouts``, ``rollout_steps`` and
    ``determinize`` as for 'rollout_agent', ``guided`` a dict with ``epsilon`` and / or ``weights`` -- None: the
    defaults); 4 x batch_size games, block i started by player i, at most
    2000 turns; a game without a legal action applies no_step.  Every game steps in its own lane each turn (a finished
    game's lane applies no_step, which leaves its pins alone), so a game's deals are keyed by its own index.  Returns
    winners[start][player] and average_progress[start][player] as the reference prints them, and their totals.
    Win-rate parity is unpinned: the reference's DOG networks and inference functions are `pass`."""
    return _four_seats(_Dog, agents, batch_size, num_simulations, max_depth, temperature, seed, rules, max_turns, greedy,
                       device, {}, report_turns=True,
                       rollout=dict(rollouts=rollouts, rollout_steps=rollout_steps, determinize=determinize),
                       guided=_guided_kwargs(guided))
