"""Self-play and batched TD updates on one GPU with no host round trips.

Learner owns one fused 1-ply Engine and one DeviceTrainer (batched, HIP) and
drives them on one stream. In the steady state no record, offset, weight or
fragment passes through host memory: the trainer reads the harvest ticket's own
arrays (DeviceTrainer.update_device), the episode offsets are computed on the
device (bgx_episode_offsets), and the engine's split-fp16 fragments are built
there from the trainer's flat parameters (bgx_set_weights_device). Per update
the host waits once, inside that hand-off, for 16 bytes: the check's verdict and
the two scalars (value_head.bias, the feature scale) the step launches take by
value.

Chunk c (run_chunk):
  1. step(steps_per_chunk) and harvest_enqueue() give ticket c; nothing waits.
  2. harvest_fetch(c - 1, clone=False): that ticket completed before step c
     began, so the host does not stall the GPU.
  3. If it holds at least one episode: update_device on its arrays,
     version += 1, set_weights_device(params, temperature(version), version).
  4. An empty ticket: no update, no version change.

The new weights therefore take effect from chunk c + 1: the games of chunk c
are played on parameters one update old. The lag is deliberate (it is what
keeps the GPU busy while the host looks at ticket c - 1), and the reference's
workers play on stale parameters too (worker.py:66-76 refreshes them between
episodes only). Ticket c - 1's arrays are read before the second enqueue after
it, as the harvest contract requires.

Episode order within a harvest is the device's completion order (the fused
engine's workgroups append as they finish), and the update sums in that order:
by default two runs of one seed play the same games in chunk 0 but do not repeat
bit for bit afterwards. deterministic=True removes that: before the update,
ticket c - 1 is put into the canonical order of ops.canonical_harvest (by lane,
then by episode number) on the learner's stream, into buffers the learner owns,
and the trainer reads those. The set of episodes in a ticket is fixed by the
seed, so a run is then a pure function of the learner's arguments: digest()
repeats to the bit from run to run, and on_update's headers / records are the
canonical arrays (the ticket's own are raw_headers / raw_records), valid until
the next update. The canonical launches OR what they find wrong with the headers
into a status word on the device; sync() reads it and raises BgxError when it is
not zero, so no update waits for it. balance=True hands out lane-steps by
ticket, so its games depend on timing: it cannot be combined.

A hand-off the scheme cannot hold (non-finite weights, |w| past the split-fp16
limit) raises BgxError; the engine keeps its previous network and can go on
stepping.
"""
from __future__ import annotations

import collections
import hashlib

import torch

from . import ops
from ._lib import BgxError
from .engine import Engine
from .net import BackgammonPolicyNetwork
from .trainer import GAMMA, GRAD_CLIP_THRESHOLD, LEARNING_RATE, DeviceTrainer


def reference_temperature(version):
    """ParameterManager.get_temperature (parameter_manager.py:79-111): 1.5 up to
    version 1, then linear to 0.5 at version 4001."""
    v = int(version)
    return 1.5 if v <= 1 else (0.5 if v >= 4001 else 1.5 - (v - 1) / 4000)


class _Params:
    """The parameter manager the trainer is built on: versioned host weights."""

    def __init__(self, sd):
        self.sd, self.version = {k: torch.as_tensor(v).detach().cpu().clone() for k, v in sd.items()}, 1

    def get_parameters(self, device=None):
        return {k: v.to(device) if device else v for k, v in self.sd.items()}

    def set_parameters(self, sd):
        self.sd = {k: v.detach().cpu().clone() for k, v in sd.items()}
        self.version += 1


def _state_dict_from(weights, seed):
    if weights is None:   # the reference's initialisation, from the learner's seed
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(int(seed))
            return BackgammonPolicyNetwork().state_dict()
    from .ops import weights_from
    W1, b1, w2, b2 = weights_from(weights)
    return {"fc1.weight": torch.from_numpy(W1.copy()), "fc1.bias": torch.from_numpy(b1.copy()),
            "value_head.weight": torch.from_numpy(w2.copy()).reshape(1, 128),
            "value_head.bias": torch.from_numpy(b2.copy()).reshape(1)}


class Learner:
    def __init__(self, lanes, steps_per_chunk, seed=0, weights=None, lam=0.0, zero_sum=False, afterstates=False,
                 lr=LEARNING_RATE, gamma=GAMMA, grad_clip=GRAD_CLIP_THRESHOLD, temperature=reference_temperature,
                 balance=False, on_update=None, device=None, deterministic=False):
        if deterministic and balance:
            raise ValueError("deterministic=True needs balance=False: the balanced launch hands out lane-steps by "
                             "ticket, so the games themselves depend on timing")
        self.deterministic = bool(deterministic)
        self.engine = Engine(lanes=lanes, seed=seed, ply=1, fused=True, balance=balance, device=device)
        if not 1 <= int(steps_per_chunk) <= self.engine.max_steps_per_call:
            raise ValueError(f"steps_per_chunk must be in 1 .. {self.engine.max_steps_per_call}")
        self.lanes, self.steps_per_chunk = int(lanes), int(steps_per_chunk)
        self.device = self.engine.device
        self.params = _Params(_state_dict_from(weights, seed))
        self.trainer = DeviceTrainer(self.params, device=self.device, lr=lr, gamma=gamma, grad_clip=grad_clip,
                                     batched=True, backend="hip", lam=lam, zero_sum=zero_sum, afterstates=afterstates)
        self.temperature = temperature
        self.on_update = on_update
        self.stream = torch.cuda.Stream(self.device)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))   # the trainer's set-up copies
        self.version = 1
        self.chunks = 0       # chunks stepped = tickets enqueued
        self.updates = 0
        self.episodes = 0     # trained episodes
        self.records = 0
        self.log = []         # (ticket, episodes, updated) of every ticket looked at
        self._timed = collections.deque()   # (kind, start event, end event), resolved once complete
        self.gpu_ms = {"step": 0.0, "update": 0.0, "canon": 0.0}
        self._canon = None    # deterministic: the canonical arrays, the workspace and the status word
        # the first network goes the host's way (there is nothing to overlap yet)
        self.engine.set_weights(self.params.get_parameters(), float(temperature(self.version)), self.version)

    # ------------------------------------------------------------ the loop
    def _mark(self):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(self.stream)
        return ev

    def _resolve(self, wait=False):
        while self._timed and (wait or self._timed[0][2].query()):
            kind, a, b = self._timed.popleft()
            if wait:
                b.synchronize()
            self.gpu_ms[kind] += a.elapsed_time(b)

    def _canonical(self, h):
        """Ticket h in canonical order, in the learner's own buffers (the current
        stream is the learner's). They grow in steps: a steady state allocates nothing."""
        n, m = h.n_episodes, h.n_records
        c = self._canon
        if c is None:
            c = self._canon = {"headers": None, "records": None, "offs": None, "work": None,
                               "status": torch.zeros(1, dtype=torch.int32, device=self.device)}
        need = ops.canonical_workspace(n, self.lanes)
        for key, rows, shape, dtype in (("headers", n, (16,), torch.int32), ("records", m, (12,), torch.int32),
                                        ("offs", n + 1, (), torch.int32), ("work", need, (), torch.uint8)):
            if c[key] is None or c[key].shape[0] < rows:
                c[key] = torch.empty((rows + rows // 4 + 16,) + shape, dtype=dtype, device=self.device)
        return ops.canonical_harvest(h.headers, h.records, lane_base=int(self.engine.cfg.lane_base), lanes=self.lanes,
                                     out=(c["headers"], c["records"], c["offs"]), status=c["status"],
                                     stream=self.stream, work=c["work"])

    def run_chunk(self):
        """One chunk of the schedule above; returns True when it made an update."""
        eng, s = self.engine, self.stream
        c = self.chunks
        a = self._mark()
        eng.step(self.steps_per_chunk, stream=s)
        self._timed.append(("step", a, self._mark()))
        ticket = eng.harvest_enqueue(stream=s)
        self.chunks = c + 1
        if c == 0:
            return False   # no earlier ticket yet
        h = eng.harvest_fetch(ticket - 1, clone=False)
        n = h.n_episodes
        self.log.append((ticket - 1, n, n > 0))
        if n == 0:
            return False
        version = self.version + 1
        temp = float(self.temperature(version))
        with torch.cuda.stream(s):   # the trainer launches on its current stream
            a = self._mark()
            headers, records, info = h.headers, h.records, {}
            if self.deterministic:
                headers, records, offs = self._canonical(h)
                b = self._mark()
                self._timed.append(("canon", a, b))
                a = b
                self.trainer.update_device(headers, records, offs=offs)
                info = {"raw_headers": h.headers, "raw_records": h.records}
            else:
                self.trainer.update_device(headers, records)
            eng.set_weights_device(self.trainer.params, temp, version, stream=s)   # raises when rejected
            self._timed.append(("update", a, self._mark()))
            self.version = version
            self.updates += 1
            self.episodes += n
            self.records += h.n_records
            if self.on_update is not None:
                self.on_update({"update": self.updates, "version": version, "temperature": temp, "chunk": c,
                                "ticket": ticket - 1, "headers": headers, "records": records, **info})
        self._resolve()
        return True

    def run(self, chunks=None, updates=None):
        """Run `chunks` chunks, or as many as it takes to make `updates` updates."""
        if (chunks is None) == (updates is None):
            raise ValueError("run(chunks=...) or run(updates=...)")
        if chunks is not None:
            for _ in range(int(chunks)):
                self.run_chunk()
        else:
            target = self.updates + int(updates)
            while self.updates < target:
                self.run_chunk()
        return self

    # ------------------------------------------------------------ the host's views, on demand
    def sync(self):
        self.stream.synchronize()
        self.engine.sync()
        self._resolve(wait=True)
        if self._canon is not None:
            bits = int(self._canon["status"].item()) & 0xFFFFFFFF
            if bits:
                what = "; ".join(v for k, v in ops.CANON_BITS.items() if bits & k)
                raise BgxError(f"canonical harvest order: status 0x{bits:x} ({what}): the updates since the last sync() "
                               f"read unspecified arrays")

    def digest(self):
        """SHA-256 (hex) of the trainer's flat parameters, Adam moments and step
        count as they stand once the stream's work is done; read on the host."""
        self.stream.synchronize()
        f = self.trainer._hip_state()
        h = hashlib.sha256()
        for key in ("p", "m", "v", "step"):
            h.update(f[key].cpu().numpy().tobytes())
        return h.hexdigest()

    def weights(self):
        """The trainer's current weights as host fp32 W1, b1, w2, b2."""
        from .ops import weights_from
        with torch.cuda.stream(self.stream):
            sd = self.trainer.state_dict()
        return dict(zip(("W1", "b1", "w2", "b2"), weights_from(sd)))

    def metrics(self, reset=True):
        with torch.cuda.stream(self.stream):
            return self.trainer.metrics(reset=reset)

    def close(self):
        self.engine.close()
