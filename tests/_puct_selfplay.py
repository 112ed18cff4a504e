"""PUCT self-play on det-MADN, restated (TEST INFRASTRUCTURE ONLY; test helper, not a test module).

``play_batch_of_games_puct`` is oracle/selfplay.py's play_batch_of_games loop (MuZero_det_MADN/game_agent.py:50-183)
with tests/_mctx_muzero.py's muzero_policy as the turn's search: what the reference plays once run_muzero_mcts'
commented mctx.muzero_policy call (muzero_deterministic_madn.py:685-697) is the live one.  All three noise streams
follow the engine's counter RNG keyed by (seed, game, the game's own step): the Dirichlet root noise through the
float32 restatement of oracle/root_noise.py, the final draw's Gumbel noise through oracle.selfplay.gumbel_noise on the
GUMBEL_STREAM, the 1e-7 tie-break uniforms inside muzero_policy.  In a batch every live game records one turn per
loop step, so the game's own step is the loop's ``step``.

``puct_selfplay_parity`` compares the engine's records with it:
  * a turn is noise-excused when one of its Gamma draws has a float64 acceptance margin below
    tests/_root_noise.threshold over the case's own draws (a comparison of the sampler may go the other way on the
    device: the whole noise row then differs), and excusable when it is noise-excused or an oracle near-tie
    (margin <= 1, tests/_parity.TIE);
  * a game is compared up to the first excusable turn at which its action or its policy row actually differs and not
    beyond; a difference at any other turn fails;
  * the turns before that point: integers and obs exactly, val and pol within 1e-5 (visit fractions: equal counts);
  * the cap, asserted on the oracle's record alone before anything is compared: the turns at or after a game's first
    excusable turn -- all that any device result could leave out -- are at most CAP = 1/3 of the recorded turns."""
import numpy as np

from oracle import detmadn as dm
from oracle import root_noise as RN
from oracle import selfplay as OS
from tests import _mctx_muzero as PZ
from tests import _root_noise as H
from tests._parity import TIE, TOL, log

A = 24
CAP = 1.0 / 3.0
EXACT_KEYS = ("act", "rew", "player", "team", "discount", "mask", "obs")


def play_batch_of_games_puct(params, root_fn, recurrent_fn, envs, num_simulations, max_depth, max_steps, temp, seed,
                             qtransform=PZ.QT_MIN_MAX, min_value=-1.0, max_value=1.0, dirichlet_fraction=0.25,
                             dirichlet_alpha=0.3, pb_c_init=1.25, pb_c_base=19652.0):
    """-> (buffers as play_batch_of_games records them, with ``margin`` [n, T] per search turn; batched turns)."""
    n = len(envs)
    envs = list(envs)
    P = envs[0].num_players
    C = dm.num_channels(P)
    T = max_steps
    teams = envs[0].rules["enable_teams"]
    buf = {
        "obs": np.zeros((n, T, C, 56), np.int8), "act": np.zeros((n, T), np.int32),
        "rew": np.zeros((n, T), np.int32), "val": np.zeros((n, T), np.float32),
        "pol": np.zeros((n, T, A), np.float32), "mask": np.zeros((n, T), np.float32),
        "player": np.zeros((n, T), np.int32), "team": np.full((n, T), -1, np.int32),
        "discount": np.zeros((n, T), np.int32), "idx": np.zeros(n, np.int32),
        "margin": np.full((n, T), np.inf),
    }
    dones = np.zeros(n, bool)
    step = 0
    while (~dones).any() and step < max_steps:
        search, nomove = [], []
        for i in range(n):
            if dones[i]:
                continue
            va = dm.valid_action(envs[i]).flatten()
            (search if va.any() else nomove).append((i, va))
        if search:
            gids = np.array([i for i, _ in search])
            obs = np.stack([dm.encode_board(envs[i]) for i in gids]).astype(np.float32)
            invalid = np.stack([~va for _, va in search])
            dirichlet = RN.root_noise(seed, gids, step, dirichlet_alpha, A, np.float32)["noise"]
            gumbel = np.stack([OS.gumbel_noise(seed ^ OS.GUMBEL_STREAM, int(g), step) for g in gids])
            lg, v, e = root_fn(params, obs)
            trace = {}
            act, w, rv, _ = PZ.muzero_policy(params, lg, v, e, recurrent_fn, num_simulations, invalid, dirichlet, gumbel,
                                             max_depth=max_depth, temperature=temp, qtransform=qtransform,
                                             min_value=min_value, max_value=max_value,
                                             dirichlet_fraction=dirichlet_fraction, pb_c_init=pb_c_init,
                                             pb_c_base=pb_c_base, seed=seed, turn=step, gids=gids, trace=trace)
            for k, i in enumerate(gids):
                env = envs[i]
                t = buf["idx"][i]
                assert t == step
                buf["margin"][i, t] = trace["margin"][k]
                cpb = env.current_player
                teamb = cpb % 2 if teams else -1
                nxt, r, nd = dm.env_step(env, dm.map_action(int(act[k])))
                nteam = nxt.current_player % 2 if teams else -1
                buf["obs"][i, t] = obs[k].astype(np.int8)
                buf["act"][i, t] = act[k]
                buf["rew"][i, t] = 2 if (nd and r > 0) else (0 if (nd and r < 0) else 1)
                buf["val"][i, t] = rv[k]
                buf["pol"][i, t] = w[k]
                buf["mask"][i, t] = 1.0
                buf["player"][i, t] = cpb
                buf["team"][i, t] = teamb
                buf["discount"][i, t] = 1 if nd else ((2 if teamb == nteam else 0) if teams
                                                      else (2 if cpb == nxt.current_player else 0))
                buf["idx"][i] = t + 1
                envs[i] = nxt
                dones[i] = nd
        for i, _ in nomove:
            env = envs[i]
            t = buf["idx"][i]
            buf["act"][i, t] = -1
            buf["rew"][i, t] = 1
            buf["player"][i, t] = env.current_player
            buf["team"][i, t] = env.current_player % 2 if teams else -1
            buf["discount"][i, t] = 1
            buf["idx"][i] = t + 1
            envs[i], _, nd = dm.no_step(env)
            dones[i] = nd
        step += 1
    return buf, step


def excusable_turns(ref, seed, dirichlet_fraction, dirichlet_alpha=0.3):
    """-> (near_tie [n, T], noise_excused [n, T]) of an oracle record."""
    near = np.isfinite(ref["margin"]) & (ref["margin"] <= TIE) & (ref["mask"] > 0)
    noise = np.zeros_like(near)
    if dirichlet_fraction > 0.0:
        gi, ti = np.nonzero(ref["mask"] > 0)           # the searches: (game, the game's own step)
        r32 = RN.root_noise(seed, gi, ti, dirichlet_alpha, A, np.float32)
        r64 = RN.root_noise(seed, gi, ti, dirichlet_alpha, A, np.float64)
        noise[gi, ti] = (r64["margin"] < H.threshold([(r32, r64)])).any(1)
    return near, noise


def first_excusable(ref, near, noise):
    """The first excusable turn of every game (its ``idx`` where it has none)."""
    idx = ref["idx"].astype(np.int64)
    ex = near | noise
    first = idx.copy()
    for i in range(len(idx)):
        t = np.flatnonzero(ex[i, :idx[i]])
        if t.size:
            first[i] = t[0]
    return first


def assert_cap(label, ref, seed, dirichlet_fraction, dirichlet_alpha=0.3, cap=CAP):
    """The cap, on the oracle's record alone.  -> (near, noise, first excusable turn per game).  (cap: only the
    CPU tests of the comparison rule itself pass another one.)"""
    near, noise = excusable_turns(ref, seed, dirichlet_fraction, dirichlet_alpha)
    first = first_excusable(ref, near, noise)
    idx = ref["idx"].astype(np.int64)
    at_or_after, turns = int((idx - first).sum()), int(idx.sum())
    log(f"{label}: searches {int((ref['mask'] > 0).sum())}, near-tie searches {int(near.sum())}, noise-excused "
        f"searches {int(noise.sum())}, games touched {int((first < idx).sum())} of {len(idx)}, turns at or after a "
        f"first excusable turn {at_or_after} of {turns} ({at_or_after / max(turns, 1):.1%}, cap {cap:.1%})")
    assert at_or_after <= cap * turns, f"{label}: {at_or_after} of {turns} turns could be left out, above the cap"
    return near, noise, first


def puct_selfplay_parity(label, buf, ref, seed, dirichlet_fraction, dirichlet_alpha=0.3, tol=TOL, cap=CAP):
    """The engine's records (buf) against the oracle's (ref).  -> the diverged games [(game, turn)]."""
    near, noise, _ = assert_cap(label, ref, seed, dirichlet_fraction, dirichlet_alpha, cap)
    ex = near | noise
    n = len(ref["idx"])
    diverged, left_out, compared, exact, max_d = [], 0, 0, 0, 0.0
    for i in range(n):
        L, Lg = int(ref["idx"][i]), int(buf["idx"][i])
        m = min(L, Lg)
        dpol = np.abs(buf["pol"][i, :m] - ref["pol"][i, :m]).max(-1) if m else np.zeros(0)
        diff = np.flatnonzero((buf["act"][i, :m] != ref["act"][i, :m]) | (dpol > tol))
        if diff.size:
            t_star = int(diff[0])
            assert ex[i, t_star], (f"{label}: game {i} differs at turn {t_star}, which is neither noise-excused nor a "
                                   f"near-tie (margin {ref['margin'][i, t_star]:.3e})")
            diverged.append((i, t_star))
            left_out += L - t_star
        else:
            assert L == Lg, f"{label}: game {i} records {Lg} turns, the oracle {L}, with equal actions"
            t_star = L
        for k in EXACT_KEYS:
            assert np.array_equal(buf[k][i, :t_star], ref[k][i, :t_star]), (label, k, i)
        if t_star:
            dv = np.abs(buf["val"][i, :t_star] - ref["val"][i, :t_star])
            assert dv.max() <= tol, f"{label}: game {i} val differs by {dv.max():.2e}"
            assert dpol[:t_star].max() <= tol
            max_d = max(max_d, float(dv.max()), float(dpol[:t_star].max()))
            s = ref["mask"][i, :t_star] > 0
            compared += int(s.sum())
            exact += int(((dpol[:t_star] == 0) & (dv == 0))[s].sum())
    log(f"{label}: {n - len(diverged)}/{n} games identical; diverged at excusable turns {diverged}; turns left out "
        f"{left_out} of {int(ref['idx'].sum())}; searches compared {compared}, bit-identical (pol and val) {exact}; "
        f"max float |d| {max_d:.2e}")
    return diverged
