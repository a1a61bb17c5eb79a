"""CPU: the one place the between-step layers are ordered (wheeledlab_amd/envs/layers.py StepLayers) over four recording stand-ins, for
every one of the 16 subsets of layers: which methods delayed / after / reset / current / adopt call, in which order and on what, with
out=None (env.step()) and with out= given (env.collect_step()); which layer fused_refusal() names; when rewrites_obs holds.  A stand-in
env without layers: step(), collect_step(), reset() and finish_collection() read `_layers` once, find None, and make the batch's own
calls alone, on the storage's own rows.  Then the span check of the layers' entry points (csrc/wl_layer_common.h) compiled for the
host as a stand-alone program (tests/host_sim/layer_spans_host.cpp), plain and under -fsanitize=address,undefined."""
import itertools
import os
import shutil
import subprocess
from types import SimpleNamespace

import pytest
import torch

from wheeledlab_amd.envs.layers import REFUSALS, StepLayers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("events", "latency", "corruption", "history")
SUBSETS = [frozenset(c) for r in range(5) for c in itertools.combinations(NAMES, r)]


class Events:
    def __init__(self, log):
        self.log = log

    def apply(self, terminated, time_outs=None):
        self.log.append(("events.apply", terminated, time_outs))

    def reset_all(self):
        self.log.append(("events.reset_all",))


class Latency:
    def __init__(self, log):
        self.log = log

    def push(self, action):
        self.log.append(("latency.push", action))
        return ("applied", action)

    def finish(self, action, row, terminated, time_outs=None):
        self.log.append(("latency.finish", action, row, terminated, time_outs))

    def reset_all(self):
        self.log.append(("latency.reset_all",))


class Corruption:
    all, row = "corruption.all", "corruption.row"

    def __init__(self, log, filled=False):
        self.log, self.filled = log, filled

    def apply(self, raw, out, reset_a, reset_b=None):
        self.log.append(("corruption.apply", raw, out, reset_a, reset_b))
        return out

    def corrupt(self, raw, reset_a, reset_b=None):
        self.log.append(("corruption.corrupt", raw, reset_a, reset_b))
        self.filled = True
        return self.row

    def adopt(self, rows):
        self.log.append(("corruption.adopt", rows))
        return self.row


class History:
    def __init__(self, log, filled=False):
        self.log, self.filled = log, filled

    def push(self, raw, reset_a, reset_b=None, fresh=False):
        self.log.append(("history.push", raw, reset_a, reset_b, fresh))
        self.filled = True
        return "history.current"

    def push_into(self, raw, prev, nxt, reset_a, reset_b=None):
        self.log.append(("history.push_into", raw, prev, nxt, reset_a, reset_b))

    def current(self):
        return "history.current"

    def adopt(self, rows):
        self.log.append(("history.adopt", rows))
        return "history.current"


def _layers(subset, filled=False):
    log = []
    made = dict(events=Events(log), latency=Latency(log), corruption=Corruption(log, filled), history=History(log, filled))
    return StepLayers(**{k: v for k, v in made.items() if k in subset}), log


@pytest.mark.parametrize("subset", SUBSETS, ids=lambda s: "+".join(n for n in NAMES if n in s) or "none")
def test_order_and_arguments_for_every_subset_of_layers(subset):
    ev, lat, cor, his = (n in subset for n in NAMES)
    L, log = _layers(subset)
    assert L.rewrites_obs == (cor or his)
    for n in NAMES:
        assert (getattr(L, n) is not None) == (n in subset)

    # before the step
    assert L.delayed("a") == (("applied", "a") if lat else "a")
    assert log == ([("latency.push", "a")] if lat else [])

    # after the step, the env's own row (step()): events -> latency finish -> corruption -> history
    del log[:]
    got = L.after("a", "raw", "T", "U")
    want = []
    if ev:
        want.append(("events.apply", "T", "U"))
    if lat:
        want.append(("latency.finish", "a", "raw", "T", "U"))       # the POLICY's action, into the step's row
    row = "raw"
    if cor:
        want.append(("corruption.corrupt", "raw", "T", "U"))
        row = "corruption.row"
    if his:
        want.append(("history.push", row, "T", "U", False))
        row = "history.current"
    assert log == want and got == row

    # after the step, into the caller's rows (collect_step()): the last layer that rewrites the row writes `out`
    del log[:]
    got = L.after("a", "raw", "T", "U", prev="prev", out="out")
    want = want[:int(ev) + int(lat)]
    if cor and not his:
        want.append(("corruption.apply", "raw", "out", "T", "U"))
    elif cor:
        want.append(("corruption.corrupt", "raw", "T", "U"))         # into the env's own row, which the push reads
    if his:
        want.append(("history.push_into", "corruption.row" if cor else "raw", "prev", "out", "T", "U"))
    assert log == want and got == ("out" if cor or his else "raw")   # nothing rewrites it: `raw` IS the caller's row

    # reset(): the raw row is read after the events and the latency have reset
    del log[:]
    got = L.reset(lambda: log.append(("raw_fn",)) or "raw", "flags")
    want = ([("events.reset_all",)] if ev else []) + ([("latency.reset_all",)] if lat else []) + [("raw_fn",)]
    row = "raw"
    if cor:
        want.append(("corruption.corrupt", "raw", "corruption.all", None))
        row = "corruption.row"
    if his:
        want.append(("history.push", row, "flags", None, True))      # (a fresh push reads no flag: any tensor of the batch)
        row = "history.current"
    assert log == want and got == row

    # current(), filled (reset() above filled them): reading runs nothing but -- with neither corruption nor history -- the raw row
    del log[:]
    got = L.current(lambda: log.append(("raw_fn",)) or "raw", "flags")
    assert got == ("history.current" if his else "corruption.row" if cor else "raw")
    assert log == ([] if cor or his else [("raw_fn",)])

    # current() before the first reset: the current state's row, every reset flag set, every frame that one
    L, log = _layers(subset)
    got = L.current(lambda: log.append(("raw_fn",)) or "raw", "flags")
    assert log == want[int(ev) + int(lat):] and got == row           # reset()'s tail, without the events and the latency
    # a corrupted row that stands is not drawn again when only the history is empty
    if cor and his:
        L, log = _layers(subset)
        L.corruption.filled = True
        assert L.current(lambda: log.append(("raw_fn",)) or "raw", "flags") == "history.current"
        assert log == [("history.push", "corruption.row", "flags", None, True)]

    # adopt(): the layer that keeps the env's row catches up; None: the batch's own row is the env's
    L, log = _layers(subset)
    got = L.adopt("rows")
    assert got == ("history.current" if his else "corruption.row" if cor else None)
    assert log == ([("history.adopt", "rows")] if his else [("corruption.adopt", "rows")] if cor else [])

    # fused_refusal(): the first layer present, in the order history, corruption, events, latency
    words = dict(history="history", corruption="corruption", events="event", latency="latency")     # what the GPU tests match on
    first = next((n for n in ("history", "corruption", "events", "latency") if n in subset), None)
    msg = L.fused_refusal()
    if first is None:
        assert msg is None
    else:
        assert msg == dict(REFUSALS)[first] + "; use step() or collect_step()" and words[first] in msg
    assert [n for n, _ in REFUSALS] == ["history", "corruption", "events", "latency"]
    assert all(words[n] in why for n, why in REFUSALS)


# ---- an env without layers ---------------------------------------------------------------------------------------------------

class _Batch:
    """a stand-in for core.EnvBatch that records what the env asks of it"""
    metrics_slots, step_count, seed, env_offset = 1, 0, 7, 0

    def __init__(self, n, D):
        self.calls = []
        self.obs = torch.zeros(n, D)
        self.reward = torch.zeros(n)
        self.terminated, self.truncated = torch.zeros(n, dtype=torch.bool), torch.zeros(n, dtype=torch.bool)
        self.metrics_raw = torch.zeros(1, 1, 32)

    def reset(self):
        self.calls.append(("reset",))

    def observe(self):
        self.calls.append(("observe",))
        return self.obs

    def step(self, action):
        self.calls.append(("step", action))
        return self.obs, self.reward, self.terminated, self.truncated

    def rollout(self, actions, obs_out, rew_out, term_out, to_out, dones_out=None):
        self.calls.append(("rollout", actions, obs_out, rew_out, term_out, to_out, dones_out))


def _bare_env(n=5, D=3):
    from wheeledlab_amd.envs.manager_based_rl_env import ManagerBasedRLEnv

    class Env(ManagerBasedRLEnv):
        reads = 0

        @property
        def _layers(self):
            Env.reads += 1
            return None

    env = Env.__new__(Env)
    env._batch = _Batch(n, D)
    env.cfg = SimpleNamespace(decimation=4, sync_episode_log=False)
    env._task, env._flat = "drift", SimpleNamespace(extra={}, curriculum=[])
    env.action_manager = SimpleNamespace(prev_action=None)
    env.common_step_counter = env._sim_step_counter = 0
    env._frame_hooks, env._has_custom_rewards, env._has_curriculum = [], False, False
    env._custom_epsum, env._custom_obs, env._custom_log = {}, [], {}
    env._log_keys, env.max_episode_length, env.max_episode_length_s = {}, 6, 1.0
    env.extras, env.obs_buf = {}, {}
    return Env, env


def _same_memory(x, y):
    return x.data_ptr() == y.data_ptr() and x.shape == y.shape and x.stride() == y.stride()


def test_an_env_without_layers_tests_one_name_and_makes_the_batch_calls_alone():
    n, D, K = 5, 3, 2
    Env, env = _bare_env(n, D)
    b = env._batch

    obs, extras = env.reset()
    assert Env.reads == 1 and b.calls == [("reset",), ("observe",)] and obs["policy"] is b.obs and extras == {}

    Env.reads, b.calls = 0, []
    action = torch.ones(n, 2)
    obs, rew, term, trunc, _ = env.step(action)
    assert Env.reads == 1 and len(b.calls) == 1 and b.calls[0][0] == "step" and b.calls[0][1] is action      # the policy's action, as given
    assert obs["policy"] is b.obs and rew is b.reward and term is b.terminated and trunc is b.truncated
    assert env.common_step_counter == 1 and env.action_manager.prev_action is action

    st = SimpleNamespace(n_steps=K, observations=torch.zeros(K + 1, n, D), actions=torch.zeros(K, n, 2), mu=torch.zeros(K, n, 2),
                         actions_log_prob=torch.zeros(K, n), values=torch.zeros(K + 1, n), rewards=torch.zeros(K, n),
                         terminated=torch.zeros(K, n, dtype=torch.bool), time_outs=torch.zeros(K, n, dtype=torch.bool),
                         dones=torch.zeros(K, n, dtype=torch.int64))
    acted = []
    policy = SimpleNamespace(act=lambda *a, **kw: acted.append((a, kw)))
    for k in range(K):
        Env.reads, b.calls = 0, []
        env.collect_step(policy, st, k)
        assert Env.reads == 1 and len(b.calls) == 1 and len(acted) == k + 1
        name, acts, obs_out, rew_out, term_out, to_out, dones_out = b.calls[0]
        assert name == "rollout"
        # the storage's own rows, one step of them: the action row the policy wrote, the step's row straight into row k + 1
        for got, want in ((acts, st.actions[k:k + 1]), (obs_out, st.observations[k + 1:k + 2]), (rew_out, st.rewards[k:k + 1]),
                          (term_out, st.terminated[k:k + 1]), (to_out, st.time_outs[k:k + 1]), (dones_out, st.dones[k:k + 1])):
            assert _same_memory(got, want)
    assert env.common_step_counter == 1 + K

    Env.reads, b.calls = 0, []
    st.observations[K].fill_(3.0)
    env.finish_collection(st)
    assert Env.reads == 1 and b.calls == []
    assert env.obs_buf["policy"] is b.obs and bool((b.obs == 3.0).all())                                     # the batch's own row caught up

    Env.reads = 0
    assert env._fused_refusal() is None and Env.reads == 1


# ---- the span check of the entry points, on the host -----------------------------------------------------------------------

SPANS_SRC = os.path.join(ROOT, "tests", "host_sim", "layer_spans_host.cpp")
CLANG = os.environ.get("WL_HOST_CXX", "/opt/rocm/lib/llvm/bin/clang++")
SPAN_CASES = {
    "disjoint": 0,
    "touching_end_to_start": 0,
    "one_byte_stored_then_read": 1,
    "one_byte_read_then_stored": 1,
    "null_read_span": 0,
    "null_stored_span": 0,
    "stored_on_a_later_read_span": 1,
    "stored_on_stored": 1,
    "read_on_read": 0,                      # allowed: only what the launch stores is held against the rest
    "null_tail": 0,
    "used_entry_behind_null_ones": 1,
    "contained": 1,
    "single_bytes_outside": 0,
    "single_byte_inside": 1,
}


@pytest.mark.parametrize("flags", [(), ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "sanitized"])
def test_span_check_on_hand_made_cases(tmp_path, flags):
    cxx = CLANG if (os.path.exists(CLANG) or shutil.which(CLANG)) else shutil.which("g++")
    if cxx is None:
        pytest.skip("no C++ compiler to build the host simulation")
    exe = str(tmp_path / "layer_spans_host")
    subprocess.run([cxx, "-O1", "-std=c++17", *flags, "-I", os.path.join(ROOT, "tests", "host_sim", "hip_stub"),
                    "-I", os.path.join(ROOT, "wheeledlab_amd", "csrc"), SPANS_SRC, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True)
    assert out.stderr == ""
    got = dict((name, int(v)) for name, v in (line.split() for line in out.stdout.splitlines()))
    assert got == SPAN_CASES
