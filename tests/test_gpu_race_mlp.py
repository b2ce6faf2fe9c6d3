"""The race modes (nascar_set_race) with MLP drivers in the field: the park mask of the MLP launches (race_park_kernel
after launch_field's launch groups and after policy 2's actor, csrc/nascar_race.h), the genome driver's parking on the
sharded block-map path (policy 5), policies 1 and 3 of policy_actions under the time trial, the ledger fed by trained
SAC / PPO / A2C cars (lap events, ties between two slots of one controller, an env that ends after lap events) and
nascargymnasium_amd.race with MLP slots.

Every comparison is exact (bits; NaN by bits).  Both sides take their MLP actions from the same device kernels: the
reference is the host loop of tests/race_ref.py fed from reward, info_tensor() and env_flags of a twin engine with race
mode off, which masks the parked cars' actions itself.  Device MLP actions differ from NumPy's in the last bits, so the
step numbers of the CPU oracle (tests/test_race_mlp_cpu.py) are not the device's: every test asserts its preconditions on
the device run itself and prints what it saw; the docstrings give both.  The step caps come from race_mlp_cases, where
the CPU test proves them."""
import numpy as np
import pytest

import race_mlp_cases as rc
import race_ref
from race_ref import F
from race_mlp_cases import FULL_THROTTLE_DISABLED_AT, P2_STEPS, PARK_STEPS, STUCK_DISABLED_AT, TT_STEPS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import test_gpu_race as R                                    # noqa: E402  (its helpers, not its tests)
from test_gpu_race import _assert_ledger, _assert_rank, _bits, _ctl, _engine, _host_rows, _set_ctl, _state_without_ctl  # noqa: E402
from test_gpu_field import _fixture, _sac_1235               # noqa: E402
from nascargymnasium_amd import _lib, genetic as G, race     # noqa: E402

SEED, GENOME_SEED = R.SEED, R.GENOME_SEED
MARGIN = 50          # steps between a precondition's event and the end, as tests/test_gpu_race.py
BUILTIN = ("rule", "noisy", "genome", "uniform")
CONTROLLERS = {"SAC": lambda: _sac_1235()[0], "PPO": lambda: _fixture("ppo_849")[0],
               "A2C": lambda: _fixture("a2c_best_model3")[0], "F": rc.full_throttle, "M": rc.wide}
MLP = tuple(CONTROLLERS)


def _genomes(E, C, idle=(), rule=()):
    """random genomes with the steering gain capped at 1 (the drivers' state is then the four control-state words alone);
    idle: envs whose cars stand on the grid (g[2] = g[3] = 0); rule: (env, slot) pairs that take RULE_GENOME, the genome
    under which the driver is the rule driver"""
    g = G.random_genomes(np.random.default_rng(GENOME_SEED), E * C).reshape(E, C, 12)
    g[:, :, 4] = np.minimum(g[:, :, 4], 1.0)
    for e, c in rule:
        g[e, c] = G.RULE_GENOME
    for e in idle:
        g[e, :, 2] = 0.0
        g[e, :, 3] = 0.0
    return g


def _mlp_engine(E, C, tracks, field=None, genomes=None, epb=None, actor=False):
    """an engine with 4 rollout streams; field: per slot a built-in name or a key of CONTROLLERS (one id per key, so two
    slots of one key share a controller)"""
    env = _engine(E, C, tracks)
    if genomes is not None:
        env.set_genomes(genomes)
    if field is not None:
        ids = {}
        for name in field:
            if name not in BUILTIN and name not in ids:
                ids[name] = env.add_controller(CONTROLLERS[name]())
        env.set_car_controllers([ids.get(name, name) for name in field])
    if actor:
        env.set_actor(_sac_1235()[1])
    env.reset()
    if epb is not None:
        env.set_envs_per_block(epb)
    return env


def _host_step(b, races, k, mode, policy):
    """tests/test_gpu_race.py's _host_step for any action source: the twin's actions, (0, 0) for the cars the time trial
    does not drive, env.step, and the reference's bookkeeping from reward, info and the env flags"""
    a = b.policy_actions(policy, SEED, k)
    if mode == 2:
        mask = torch.from_numpy(np.array([r.parked() for r in races])).cuda()
        a = a.clone()
        a[mask] = 0.0
    b.step(a, auto_reset=False)
    rew, info = b.reward.cpu().numpy(), b.info_tensor().cpu().numpy()
    done = (b.env_flags.cpu().numpy() & (_lib.EF_TERMINATED | _lib.EF_TRUNCATED)) != 0
    laps, last, dis, st = R._info_cols(info)
    for e, r in enumerate(races):
        if not r.ended:
            r.step(rew[e], laps[e].tolist(), [race_ref.none_if_nan(x) for x in last[e]], dis[e].tolist(), float(st[e, 0]),
                   bool(done[e]))


def _host_attempt(b, races, policy, K, step0=0):
    """K steps of the twin's time-trial attempt.  Returns parked_at [E, C], ended_at [E] (steps, 0: never) and the
    control-state row each parked car had when it parked (the reference does not call a parked car's controller)."""
    E, C = b.E, b.C
    parked_at, ended_at, frozen = np.zeros((E, C), np.int64), np.zeros(E, np.int64), {}
    for k in range(K):
        before = [r.parked() for r in races]
        _host_step(b, races, step0 + k, 2, policy)
        new = [(e, n) for e, r in enumerate(races) for n, p in enumerate(r.parked()) if p and not before[e][n]]
        if new:
            ctl = _ctl(b).reshape(E, C, 4)
            for e, n in new:
                frozen[(e, n)] = ctl[e, n].copy()
                parked_at[e, n] = k + 1
        for e, r in enumerate(races):
            if r.ended and not ended_at[e]:
                ended_at[e] = k + 1
    return parked_at, ended_at, frozen


def _assert_same_attempt(a, b, races, frozen, what):
    """the device attempt against the twin's: ledger, fastest_car, ended, rank, obs, state, and the control state with the
    parked cars' rows frozen.  Puts the frozen rows back into the twin (the next attempt starts from them)."""
    E, C = a.E, a.C
    led, fastest, ended = _host_rows(races)
    dev = a.race()
    _assert_ledger(dev.ledger.cpu().numpy(), led, what)
    assert np.array_equal(dev.fastest_car.cpu().numpy(), fastest), what
    assert np.array_equal(dev.ended.cpu().numpy(), ended), what
    assert torch.equal(a.obs, b.obs), what
    assert torch.equal(_state_without_ctl(a), _state_without_ctl(b)), (what, R._state_diff(a, b))
    want_ctl = _ctl(b).reshape(E, C, 4).copy()
    for (e, n), row in frozen.items():
        want_ctl[e, n] = row
    assert np.array_equal(_bits(_ctl(a)), _bits(want_ctl.reshape(E * C, 4))), what
    _assert_rank(a, 2, led, fastest, what)
    _set_ctl(b, want_ctl)
    return led, fastest


def _same_run(a, c, what):
    """two device engines after the same run: obs, the whole state and the ledger by bits"""
    assert torch.equal(a.obs, c.obs) and torch.equal(a.get_state(), c.get_state()), what
    ra, rc_ = a.race(), c.race()
    assert torch.equal(ra.ledger.view(torch.int64), rc_.ledger.view(torch.int64)), what
    assert torch.equal(ra.fastest_car, rc_.fastest_car) and torch.equal(ra.ended, rc_.ended), what


def _u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ------------------------------------------------------------------ 1. the park mask by itself
PARK_FIELD = ["F", "rule", "SAC", "genome", "F", "noisy", "M"]


@pytest.mark.parametrize("E,C", [(1, 1), (37, 7), (4, 64), (5, 51), (9, 29)])
def test_park_mask_at_edge_shapes(E, C):
    """N = 1, 259, 256, 255, 261 cars: one lane, and one car past / exactly at / one short of / five past a 256-lane block
    of race_park_kernel, policy_kernel and the genome kernel.  Odd envs on martinsville, even ones on daytona (the single
    env of 1 x 1 on martinsville, so that its one car is a parked one); the slots cycle through PARK_FIELD; every third
    env's genomes idle.  After rollout(4, 450) under the time trial the ledger's parked column is set for exactly the F
    slots of the martinsville envs: the (1, 0) controller is disabled there at step 404 (bit-exact on any kernel: CPU
    oracle and device agree) and nothing else is disabled within 450 steps.  A twin with race mode off takes the state and
    the observation; for policies 4, 5, 1, 3 and 2 the parked rows of policy_actions are +0.0, every other row is the
    twin's, the parked cars' control state is untouched and every other car's is the twin's."""
    tracks = ["martinsville" if e % 2 or E == 1 else "daytona" for e in range(E)]
    field = [PARK_FIELD[c % len(PARK_FIELD)] for c in range(C)]
    g = _genomes(E, C, idle=[e for e in range(E) if e % 3 == 2])
    a, b = (_mlp_engine(E, C, tracks, field, g, actor=True) for _ in range(2))
    a.set_race(2, 1)
    a.rollout(4, PARK_STEPS, seed=SEED, auto_reset=False)
    led = a.race().ledger.cpu().numpy()
    parked = led[..., F["parked"]] != 0
    want = np.array([[tracks[e] == "martinsville" and field[c] == "F" for c in range(C)] for e in range(E)])
    assert np.array_equal(parked, want), np.argwhere(parked != want)[:8].tolist()
    assert (led[..., F["disabled"]] != 0)[want].all()
    ended = want.all(1)             # (the single car of 1 x 1: its attempt ended with the step that parked it)
    assert (led[~ended][..., F["steps"]] == PARK_STEPS).all() and (led[ended][..., F["steps"]] == FULL_THROTTLE_DISABLED_AT).all()
    assert want.any() and (E == 1 or (want[0] != want[1]).any())        # the mask differs between envs
    b.set_state(a.get_state())
    b.obs.copy_(a.obs)
    pk = want.reshape(-1)
    for p in (4, 5, 1, 3, 2):
        ctl_a0, ctl_b0 = _ctl(a).copy(), _ctl(b).copy()
        A = a.policy_actions(p, SEED, PARK_STEPS).cpu().numpy().reshape(-1, 2)
        B = b.policy_actions(p, SEED, PARK_STEPS).cpu().numpy().reshape(-1, 2)
        ctl_a, ctl_b = _ctl(a), _ctl(b)
        assert (_u32(A[pk]) == 0).all(), (p, A[pk][:4])                          # parked rows: (+0.0, +0.0)
        assert (_u32(B[pk]) != 0).any(), p                                       # which the source itself does not write
        assert np.array_equal(_u32(A[~pk]), _u32(B[~pk])), (p, np.argwhere(_u32(A) != _u32(B))[:4].tolist())
        assert np.array_equal(_bits(ctl_a[pk]), _bits(ctl_a0[pk])), p            # a parked car's controller is not run
        assert np.array_equal(_bits(ctl_a[~pk]), _bits(ctl_b[~pk])), p
        if p in (5, 1, 3):          # the built-in drivers keep state: the twin's rows of the parked cars did move
            assert not np.array_equal(_bits(ctl_b[pk]), _bits(ctl_b0[pk])), p
            assert E == 1 or not np.array_equal(_bits(ctl_a[~pk]), _bits(ctl_a0[~pk])), p
    a.close(); b.close()


# ------------------------------------------------------------------ 2. time trial of a mixed MLP field, policy 4
TT_FIELD = ["SAC", "rule", "PPO", "genome", "A2C", "F", "noisy", "M"]
TT_TRACKS = ["nascar_banked"] * 4 + ["martinsville"] * 2


def test_time_trial_mixed_mlp_field():
    """4 envs on nascar_banked + 2 on martinsville, 8 cars [SAC, rule, PPO, genome, A2C, F, noisy, M], one lap per attempt,
    two attempts of 2900 steps, 3 envs per workgroup against the automatic layout: tests/test_gpu_race.py's
    test_time_trial_26x10 with three MLP launch groups (256-256 ReLU; 64-64 Tanh with two slots, PPO and F; 256-128 ReLU)
    and the wide kernel in the field, so the park mask follows several launches and precedes the built-in slots' kernels.
    Env 3's genomes idle; the martinsville envs' genome slot holds RULE_GENOME, without which no env of this field ends an
    attempt (CPU oracle: the random genomes of slot 3 neither lap nor crash within 2900 steps on either track).
    CPU oracle, attempt 1 (float32 NumPy actions): on nascar_banked A2C laps at step 2588, SAC at 2595, PPO at 2611, rule
    at 2828, M (whose arg max stands still) is disabled at 600 and F at 1968; on martinsville F is disabled at 404, M at
    600, SAC at 783, A2C at 1118, PPO at 1172, rule laps at 1679 and noisy at 1840 / 1978.
    Device (MI355X), both attempts: on nascar_banked SAC laps at 2595, A2C at 2601, PPO at 2618, F is disabled at 1968, M
    at 600; on martinsville SAC is disabled at 675, A2C at 700, PPO at 1172, F at 404, M at 600 -- the trained nets'
    crashes come earlier than NumPy's, the laps within 13 steps of it.  The built-in slots equal the oracle's: attempt 1
    rule 2828 / 1679 and noisy 1840 / 1978, so envs 4 and 5 end there; attempt 2 starts from the control state the cars
    parked with: rule laps at 1708 on martinsville and not within 2900 steps on nascar_banked, env 4's noisy car laps at
    1971, and env 5's, which parked braking (throttle -1), rolls back over the line at step 4 and is disabled by the
    backward rule, as the CPU oracle's is.  Fastest car: A2C in the nascar_banked envs, rule on martinsville.
    F is meant to be parked in the martinsville envs only, which makes the mask differ between envs; since the
    full-throttle car also leaves nascar_banked (at 1968, before any trained car can lap there) that holds until then,
    not at the end of an attempt: asserted as F parked at step 404 exactly in the martinsville envs and not within the
    CPU test's 900 steps elsewhere."""
    E, C, K = 6, 8, TT_STEPS
    g = _genomes(E, C, idle=[3], rule=[(4, 3), (5, 3)])
    a, b, c = (_mlp_engine(E, C, TT_TRACKS, TT_FIELD, g, epb) for epb in (3, None, None))
    a.set_race(2, 1)
    c.set_race(2, 1)
    races = [race_ref.EnvRace(C, 2, 1) for _ in range(E)]
    mlp_slots = [i for i, name in enumerate(TT_FIELD) if name in MLP]
    banked, mville = [0, 1, 2, 3], [4, 5]
    for att in range(2):
        a.race_begin(keep_records=att > 0)
        a.reset()
        a.rollout(4, K, seed=SEED, step0=att * K, auto_reset=False)
        b.reset()
        for r in races:
            r.begin(att > 0)
        parked_at, ended_at, frozen = _host_attempt(b, races, 4, K, att * K)
        led, fastest = _assert_same_attempt(a, b, races, frozen, att)
        if att == 0:
            c.race_begin(False)
            for k in range(K):
                c.step(c.policy_actions(4, SEED, k), auto_reset=False)
            _same_run(a, c, "policy_actions(4) + step under mode 2")
        print("attempt", att, "ended at", ended_at.tolist(), "parked at", parked_at.tolist(), "fastest", fastest.tolist())
        end = np.where(ended_at > 0, ended_at, K)
        lapped = led[..., F["attempt_laps"]] == 1
        early = (parked_at > 0) & (parked_at <= end[:, None] - MARGIN)
        assert any(lapped[e, 0] and early[e, 0] and lapped[e, 2] and early[e, 2] for e in banked)   # a SAC and a PPO car
        assert (parked_at[mville, 5] == FULL_THROTTLE_DISABLED_AT).all()                        # F: martinsville only,
        assert ((parked_at[banked, 5] == 0) | (parked_at[banked, 5] > 900)).all()               # for as long as it can be
        assert (led[mville, 5, F["disabled"]] == 1).all() and (led[mville, 5, F["attempt_laps"]] == 0).all()
        assert ((ended_at > 0) & (ended_at < K)).any() and (ended_at == 0).any()
        assert frozen and (led[..., F["attempt_laps"]] <= 1).all()
    assert (led[:, mlp_slots, F["laps_timed"]] >= 2).any()
    for env in (a, b, c):
        env.close()


# ------------------------------------------------------------------ 3. policy 2 under the race modes
P2_TRACKS = ["nascar_banked"] * 3 + ["martinsville"] * 2


def test_policy_2_time_trial_and_competition():
    """set_actor(sac_1235), 3 nascar_banked + 2 martinsville envs of 3 cars, 2 envs per workgroup, one lap:
    rollout(2, K) under mode 2 against the twin's policy_actions(2) + host mask + step, against a third engine's
    policy_actions(2) + step under mode 2, and against itself with one rollout stream.  launch_actions writes the actor's
    rows through act + c0 * 2 and the mask through absolute car indices.  CPU oracle: every nascar_banked car laps at
    step 2595 (three slots of one controller from one grid point: a best-lap and fastest-lap tie that car 0 takes),
    every martinsville car is disabled at 783.  Device: 2595 for all nine nascar_banked cars, whose envs end there, and 675
    on martinsville; the precondition's "50 steps before the end" is the end of the rollout, which goes on masking an
    ended env's cars.  Then the same engines in mode 1 over 1300 steps: the martinsville envs terminate once their three
    cars are disabled (device: step 675) and their rows freeze while the others go on."""
    E, C, K = 5, 3, P2_STEPS
    a, b, c = (_mlp_engine(E, C, P2_TRACKS, None, None, epb, actor=True) for epb in (2, None, None))
    a.set_race(2, 1)
    c.set_race(2, 1)
    a.race_begin(False)
    a.rollout(2, K, seed=SEED, auto_reset=False)
    races = [race_ref.EnvRace(C, 2, 1) for _ in range(E)]
    parked_at, ended_at, frozen = _host_attempt(b, races, 2, K)
    led, fastest = _assert_same_attempt(a, b, races, frozen, "policy 2")
    print("policy 2 time trial: ended at", ended_at.tolist(), "parked at", parked_at.tolist(), "fastest", fastest.tolist())
    c.race_begin(False)
    for k in range(K):
        c.step(c.policy_actions(2, SEED, k), auto_reset=False)
    _same_run(a, c, "policy_actions(2) + step under mode 2")
    a.set_rollout_streams(1)
    a.race_begin(False)
    a.reset()
    a.rollout(2, K, seed=SEED, auto_reset=False)
    _same_run(a, c, "one rollout stream")
    a.set_rollout_streams(4)
    lapped, disabled = led[..., F["attempt_laps"]] == 1, led[..., F["disabled"]] == 1
    early = (parked_at > 0) & (parked_at <= K - MARGIN)              # (the rollout masks an ended env's cars until K)
    assert (lapped & early)[:3].any()                                # a nascar_banked car parked by a lap, 50 steps early
    assert (disabled & ~lapped & (parked_at > 0))[3:].any()          # a martinsville car parked by disabling
    assert ((parked_at == 0) | (parked_at > K // 2)).any()           # an unparked car at K // 2
    assert (fastest[:3] == 0).all()                                  # the tie goes to the lowest index
    # ---- competition
    K1 = 1300
    a.set_race(1)
    a.race_begin(False)
    a.reset()
    b.reset()
    a.rollout(2, K1, seed=SEED, auto_reset=False)
    races = [race_ref.EnvRace(C, 1) for _ in range(E)]
    ended_at = {}
    for k in range(K1):
        _host_step(b, races, k, 1, 2)
        for e, r in enumerate(races):
            if r.ended:
                ended_at.setdefault(e, k + 1)
    led, fastest, ended = _host_rows(races)
    dev = a.race()
    assert torch.equal(a.obs, b.obs) and torch.equal(a.get_state(), b.get_state())
    _assert_ledger(dev.ledger.cpu().numpy(), led, "competition, policy 2")
    assert np.array_equal(dev.fastest_car.cpu().numpy(), fastest) and np.array_equal(dev.ended.cpu().numpy(), ended)
    _assert_rank(a, 1, led, fastest, "competition, policy 2")
    print("policy 2 competition: ended at", ended_at)
    assert sorted(ended_at) == [3, 4] and all(k <= K1 - MARGIN for k in ended_at.values())
    for e, k in ended_at.items():
        assert (led[e, :, F["steps"]] == k).all()                    # frozen at the terminal step for >= 50 further steps
    assert (led[:3, :, F["steps"]] == K1).all() and a.race_racing() == 3
    for env in (a, b, c):
        env.close()


def test_policy_2_park_mask_on_shards():
    """One track, so the block map is the identity and rollout(2) really runs as four shards whose cars start at
    c0 = 0, 6, 12, 18 (8 martinsville envs of 3 cars, 2 envs per workgroup): each shard's park launch must read the
    ledger's parked field at its own absolute car indices.  Thirty uniform-random steps before the race scatter the
    cars, so the SAC actor crashes them at different steps and the shards' masks differ.  Against a second engine's
    policy_actions(2) + step under mode 2 (whose one launch starts at car 0), which also records when each car parked
    (device: 14 of the 24 cars between steps 549 and 870, at 12 different steps)."""
    E, C, K = 8, 3, 900
    a, c = (_mlp_engine(E, C, "martinsville", None, None, 2, actor=True) for _ in range(2))
    a.rollout(0, 30, seed=SEED, auto_reset=False)
    c.set_state(a.get_state())
    c.obs.copy_(a.obs)
    for env in (a, c):
        env.set_race(2, 1)
        env.race_begin(False)
    a.rollout(2, K, seed=SEED, auto_reset=False)
    parked_at = np.zeros(E * C, np.int64)
    for k in range(K):
        c.step(c.policy_actions(2, SEED, k), auto_reset=False)
        now = c.race().ledger[..., F["parked"]].cpu().numpy().reshape(-1) != 0
        parked_at[now & (parked_at == 0)] = k + 1
    print("parked at", parked_at.reshape(E, C).tolist())
    _same_run(a, c, "four shards")
    # a car of a later shard that parked at another step than the car at the same offset into shard 0
    n0 = np.repeat(np.arange(E) // 2 * 2 * C, C)
    n = np.arange(E * C)
    assert (parked_at > 0).any() and (parked_at[n] != parked_at[n - n0])[n0 > 0].any()
    a.close(); c.close()


# ------------------------------------------------------------------ 4. policy 5 under the time trial, sharded
def test_policy_5_time_trial_on_the_block_map_path():
    """14 martinsville envs of 10 genome cars, 12 envs per workgroup (two workgroups, so two shards of 12 and 2 envs),
    rollout(5, 1800) under mode 2: each shard's genome launch walks its env slots of the block map (slot0 >= 0), the only
    way into genome_policy_kernel<true> on that path, against the twin's policy_actions(5) + mask + step.  Slot 0 of every
    env holds RULE_GENOME (the rule driver: CPU oracle lap at step 1680); env IDLE_ENV stands on the grid and is
    disabled by the stuck rule at 600, which ends its attempt.  Device: slot 0 laps at step 1679 in the 13 driving
    envs, 40 of the 140 cars are parked at step 1800 and only the idle env has ended."""
    E, C, K, idle = 14, 10, 1800, R.IDLE_ENV
    g = _genomes(E, C, idle=[idle], rule=[(e, 0) for e in range(E)])
    a, b = (_mlp_engine(E, C, "martinsville", None, g, epb) for epb in (12, None))
    a.set_race(2, 1)
    a.race_begin(False)
    a.rollout(5, K, seed=SEED, auto_reset=False)
    races = [race_ref.EnvRace(C, 2, 1) for _ in range(E)]
    parked_at, ended_at, frozen = _host_attempt(b, races, 5, K)
    led, fastest = _assert_same_attempt(a, b, races, frozen, "policy 5")
    print("policy 5: ended at", ended_at.tolist(), "slot 0 parked at", parked_at[:, 0].tolist(),
          "cars parked", int((parked_at > 0).sum()))
    end = np.where(ended_at > 0, ended_at, K)
    lapped, disabled = led[..., F["attempt_laps"]] == 1, led[..., F["disabled"]] == 1
    assert (lapped & (parked_at > 0) & (parked_at <= end[:, None] - MARGIN)).any()      # parked by a lap, 50 steps early
    assert (disabled & ~lapped & (parked_at > 0)).any()                                 # parked by disabling
    assert ended_at[idle] == STUCK_DISABLED_AT and (parked_at[idle] == STUCK_DISABLED_AT).all()
    assert (ended_at == 0).any() and (parked_at == 0).any()
    assert (parked_at[12:] > 0).any()                                                   # also in the second shard
    a.close(); b.close()


# ------------------------------------------------------------------ 5. a competition that ends an env after lap events
def _competition_after_laps(tracks, K, chunk):
    E, C = 2, 3
    field = ["SAC", "PPO", "A2C"]
    a, b = _mlp_engine(E, C, tracks, field, None, 1), _mlp_engine(E, C, tracks, field)
    a.set_race(1)
    races = [race_ref.EnvRace(C, 1) for _ in range(E)]
    ended_at = {}
    for k0 in range(0, K, chunk):
        a.rollout(4, chunk, seed=SEED, step0=k0, auto_reset=False)
        for k in range(k0, k0 + chunk):
            _host_step(b, races, k, 1, 4)
            for e, r in enumerate(races):
                if r.ended:
                    ended_at.setdefault(e, k + 1)
        led, fastest, ended = _host_rows(races)
        dev = a.race()
        _assert_ledger(dev.ledger.cpu().numpy(), led, k0)
        assert np.array_equal(dev.fastest_car.cpu().numpy(), fastest) and np.array_equal(dev.ended.cpu().numpy(), ended)
    assert torch.equal(a.obs, b.obs) and torch.equal(a.get_state(), b.get_state())
    _assert_rank(a, 1, led, fastest, "competition")
    # 50 further steps on the device: the ended env's rows, fastest car and order stay; the other env's rows move
    before = a.race()
    a.rollout(4, MARGIN, seed=SEED, step0=K, auto_reset=False)
    after = a.race()
    for e in range(E):
        same = torch.equal(before.ledger[e].view(torch.int64), after.ledger[e].view(torch.int64))
        assert same == (e in ended_at), e
    assert torch.equal(before.fastest_car[list(ended_at)], after.fastest_car[list(ended_at)])
    a.close(); b.close()
    return led, fastest, ended_at


def test_competition_ends_an_env_after_lap_events():
    """nascar2 and nascar_banked, [SAC, PPO, A2C], mode 1, rollout(4) in chunks of 400 against the host loop over 6400
    steps.  CPU oracle on nascar2: SAC is disabled at step 597, A2C at 1748, PPO times laps at 2656 and 4934 and is
    disabled at 6166, where the env terminates.  Device: the nascar2 env terminates at step 2782 with one timed lap, A2C's
    (its path there is chaotic), and PPO disabled before lapping; every nascar_banked car has timed two laps by 6400 and
    SAC holds that env's fastest.  Either way an env that ends after lap events, with a fastest-lap holder, while the
    other env races on; its rows then stay for 50 further device steps."""
    K = 6400
    led, fastest, ended_at = _competition_after_laps(["nascar2", "nascar_banked"], K, 400)
    print("ended at", ended_at, "laps timed", led[..., F["laps_timed"]].tolist(), "fastest", fastest.tolist())
    assert list(ended_at) == [0] and ended_at[0] <= K - MARGIN
    assert (led[0, :, F["laps_timed"]] > 0).any() and fastest[0] >= 0
    assert (led[0, :, F["steps"]] == ended_at[0]).all() and (led[0, :, F["disabled"]] == 1).all()
    assert (led[1, :, F["steps"]] == K).all()


# ------------------------------------------------------------------ 6. race.py with MLP slots
def _race_engine(E, tracks, field, g):
    C = len(field)
    env = _mlp_engine(E, C, tracks, field, g, actor=True)
    return env


def test_championship_with_mlp_slots_equals_per_track_stages():
    """tests/test_gpu_race.py's test_championship_equals_per_track_stages with the field [genome, PPO, SAC] on
    nascar_banked and martinsville: one engine of 2 tracks x 2 replicas == per-track engines, key by key, and the table
    added up the same way."""
    tracks, Rp, field = ["nascar_banked", "martinsville"], 2, ["genome", "PPO", "SAC"]
    C = len(field)
    g = _genomes(4, C)
    kw = dict(attempts=2, laps=1, chunk=128)
    env = _race_engine(4, "nascar_banked", field, g)
    table, tt, comp = race.championship(env, [rc.track(t) for t in tracks], time_trial_steps=300, competition_steps=700, **kw)
    env.close()
    want = race.ChampionshipTable(Rp, C)
    for t, name in enumerate(tracks):
        one = _race_engine(Rp, name, field, g[t * Rp:(t + 1) * Rp])
        tt1 = race.time_trial(one, max_steps=300, **kw)
        comp1 = race.competition(one, max_steps=700, chunk=128)
        one.close()
        for key in ("order", "points", "ledger", "fastest_car", "ended"):
            assert np.array_equal(tt[key][t * Rp:(t + 1) * Rp], tt1[key], equal_nan=key == "ledger"), (name, key)
            assert np.array_equal(comp[key][t * Rp:(t + 1) * Rp], comp1[key], equal_nan=key == "ledger"), (name, key)
        want.add_time_trial(tt1["order"], tt1["points"])
        want.add_competition(comp1["order"], comp1["points"], comp1["fastest_car"])
    assert np.array_equal(table.points, want.points)
    for key in want.stats:
        assert np.array_equal(table.stats[key], want.stats[key]), key
    assert all(np.array_equal(x, y) for x, y in zip(table.standings(), want.standings()))
    assert comp["total_reward"].std() > 0 and (comp["steps"], tt["steps"]) == (700, [300, 300])
    assert (comp["total_reward"][:, 1] != comp["total_reward"][:, 2]).all()       # PPO and SAC drove differently


@pytest.mark.parametrize("policy", [2, 5])
def test_time_trial_policies_2_and_5_split_over_two_engines(policy):
    """race.PARKING_POLICIES promises policies 2 and 5 beside 4: race.time_trial(env, policy) on 4 envs (two per track)
    equals the same call on two engines of two envs each."""
    tracks, field = ["nascar_banked"] * 2 + ["martinsville"] * 2, ["genome", "PPO", "SAC"]
    g = _genomes(4, 3)
    kw = dict(policy=policy, attempts=2, laps=1, max_steps=300, chunk=128)
    env = _race_engine(4, tracks, field, g)
    whole = race.time_trial(env, **kw)
    env.close()
    for h in range(2):
        half = _race_engine(2, tracks[2 * h:2 * h + 2], field, g[2 * h:2 * h + 2])
        part = race.time_trial(half, **kw)
        half.close()
        for key in ("order", "position", "points", "ledger", "fastest_car", "ended", "total_reward"):
            assert np.array_equal(whole[key][2 * h:2 * h + 2], part[key], equal_nan=key == "ledger"), (h, key)
        assert whole["steps"] == part["steps"] == [300, 300]
    assert (whole["ledger"][..., F["steps"]] == 300).all() and whole["total_reward"].std() > 0
