"""TD(0) trainer on device-resident episodes.

The reference's consumer (src/agents/trainer.py:10-166, Trainer.update) takes
exactly MIN_EPISODES_TO_TRAIN = 200 Episodes and, for each episode in turn:
Y = V(observations) (trainer.py:106-107), target = rewards with
gamma * Y[1:].detach() added to all but the last step (110-114), MSE loss
(117), zero_grad / backward (120-121), clip_grad_norm_(params, 1.0) (124-127),
the post-clip gradient norm as a metric (130-135), Adam step (lr 1e-3; the
configured LR decay is never applied in the reference) (138), then the new
state_dict goes to the ParameterManager (161).

DeviceTrainer.update_records() runs the same per-episode sequence straight
from the engine's compact records, and update(episodes) keeps the
reference's signature. backend="hip" (the default for records) runs the whole
update as one libbgx launch (bgx_td0_update, csrc/bgx_train.hip: weights in
registers, Adam moments in place, no host sync per episode); backend="torch"
runs it as eager torch ops (observations re-encoded with bgx_encode), the
checker the HIP path is tested against. batched=True is a flagged semantic
change: one Adam step per update on the mean of the per-episode losses. It
runs as eager torch ops unless backend="hip" is asked for explicitly, which
runs update_records as bgx_td0_update_batched (csrc/bgx_train_batch.hip: the
forward and backward passes over all CUs, episodes of any length);
bgx/train_ref.py restates that update in numpy. The three paths share the
flat state, so a trainer may change backend between updates.

lam (default 0: TD(0), the reference's target) makes the target the
lambda-return G_s = r_s + gamma ((1 - lam) Y_{s+1} + lam G_{s+1}) on the detached
Y, G = r on an episode's last record. The torch backend honours it, sequential
and batched; batched=True with backend="hip" runs bgx_tdlambda_update_batched
(the targets computed on the device, csrc/bgx_train_lambda.hip). The
sequential HIP kernel knows TD(0) only.

zero_sum (default False: the reference's target, which adds the next record's
value with a plus sign whoever moves there) makes the target agree with how the
engine uses V, the value for the player whose indicator is set: where the mover
changes from record s to s + 1, Y_{s+1} and G_{s+1} enter from the opponent's
side, as 1 - x:
    G_s = r_s + gamma ((1 - lam) B_s(Y_{s+1}) + lam B_s(G_{s+1})),
    B_s(x) = 1 - x if mover_s != mover_{s+1} else x
(consecutive records share a mover when the opponent passed). The movers come
from word 11 bit 9 of the records, or from feature 197 (the indicator of player
1) of an Episode's observations: the same bit in engine records. The torch
backend honours it, sequential and batched; batched=True with backend="hip"
runs bgx_td_update_batched with BGX_TDF_ZERO_SUM (the zero-sum instance of the
target stage, at every lam). The sequential HIP kernel stays the reference's
TD(0).

afterstates (default False: V is fitted on the board before each move, as the
reference's trainer does) fits V on the positions the engine rates instead:
record s contributes V(A_s), A_s the board after its move under the indicator
of its own mover (the next record's before-board, or the header's final board
on an episode's last record; bgx.records.packed_afterstates). The targets'
recurrence is unchanged, with Y_s = V(A_s): rewards, lam and zero_sum mean what
they mean above. The torch backend honours it, sequential and batched (on the
Episode path the row is next_observation with features 196 / 197 rewritten to
the mover's, the mover taken from the observation's feature 197);
batched=True with backend="hip" runs bgx_td_afterstate_update_batched at every
lam / zero_sum. The sequential HIP kernel stays the reference's TD(0) on
before-move positions.

update_device(headers, records) is update_records for a loop that never leaves
the device (bgx/learner.py): batched=True with backend="hip" only, device
tensors in (a harvest ticket's own arrays will do), the episode offsets from
bgx_episode_offsets, no tensor read on the host, the metrics summed in a device
tensor. metrics(), sync_module(), state_dict() and publish() bring the host's
views up to date when asked; `params` is the flat tensor
Engine.set_weights_device takes.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from .records import WIN_TYPES, packed_afterstates
from .net import BackgammonPolicyNetwork

LEARNING_RATE = 1e-3          # config/configuration.py:17
GAMMA = 0.99                  # configuration.py:15
GRAD_CLIP_THRESHOLD = 1.0     # configuration.py:18
MIN_EPISODES_TO_TRAIN = 200   # configuration.py:7


class DeviceTrainer:
    def __init__(self, parameter_manager, device=None, lr=LEARNING_RATE, gamma=GAMMA,
                 grad_clip=GRAD_CLIP_THRESHOLD, batch_episode_size=MIN_EPISODES_TO_TRAIN, batched=False,
                 backend=None, lam=0.0, zero_sum=False, afterstates=False):
        self.parameter_manager = parameter_manager
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        self.policy_network = BackgammonPolicyNetwork().to(self.device)
        sd = {k: torch.as_tensor(v).to(self.device) for k, v in parameter_manager.get_parameters().items()}
        self.policy_network.load_state_dict(sd)
        self.optimizer = torch.optim.Adam(self.policy_network.parameters(), lr=lr)
        self.gamma = torch.tensor(gamma, device=self.device)
        self.grad_clip = grad_clip
        self.batch_episode_size = batch_episode_size
        self.batched = batched
        if backend is None:   # not chosen: the sequential update on HIP, the batched one on torch
            backend = "torch" if batched else "hip"
        if backend not in ("hip", "torch"):
            raise ValueError(f"backend must be 'hip' or 'torch', not {backend!r}")
        self.backend = backend
        lam = float(lam)
        if not 0.0 <= lam <= 1.0:   # a NaN fails it too
            raise ValueError(f"lam must be in [0, 1], not {lam!r}")
        self.lam = lam
        if not isinstance(zero_sum, (bool, np.bool_)):
            raise ValueError(f"zero_sum must be a bool, not {zero_sum!r}")
        self.zero_sum = bool(zero_sum)
        if not isinstance(afterstates, (bool, np.bool_)):
            raise ValueError(f"afterstates must be a bool, not {afterstates!r}")
        self.afterstates = bool(afterstates)
        self.total_episodes = 0
        self._flat = None   # HIP backend state: params / Adam m / v (flat, state_dict order), step
        self._work = None   # batched HIP backend: the workspace tensor, regrown on demand
        self._dev = None    # update_device: the metrics accumulator, the offsets buffer and the host-side counts
        self._gamma_host = float(self.gamma)   # read once: update_device reads no device tensor

    @staticmethod
    def batch_shape():
        """(records per tile, largest grid) of the batched HIP backward launch."""
        import ctypes
        from ._lib import check, lib
        tile, grid = ctypes.c_int(0), ctypes.c_int(0)
        check(lib().bgx_td0_batch_shape(ctypes.byref(tile), ctypes.byref(grid)), "bgx_td0_batch_shape")
        return tile.value, grid.value

    # ------------------------------------------------------------ inputs
    def _host_inputs(self, headers, records):
        """What every update_records path starts from: the records as a contiguous
        int32 device tensor, the headers as host uint32, the episode lengths and
        their offsets [n + 1] (host int64). The checks are the callers'."""
        rec = torch.as_tensor(records).to(self.device)
        if rec.dtype != torch.int32:
            rec = rec.view(torch.int32) if rec.dtype == torch.uint32 else rec.to(torch.int32)
        hdr = np.asarray(torch.as_tensor(headers).cpu().numpy()).astype(np.uint32)
        lens = hdr[:, 3].astype(np.int64)
        return rec.contiguous(), hdr, lens, np.concatenate([[0], np.cumsum(lens)])

    def _from_records(self, headers, records):
        """(observations [m, 198], rewards [m], episode lengths, win types, movers [m]) on the device."""
        rec, hdr, lens, _ = self._host_inputs(headers, records)
        before = torch.zeros((rec.shape[0], 8), dtype=torch.int32, device=self.device)
        if self.afterstates:   # the board after the move, the mover's indicator (records.packed_afterstates)
            rows = packed_afterstates(np.asarray(torch.as_tensor(headers).cpu().numpy()), rec.cpu().numpy())
            before[:, :7] = torch.from_numpy(rows[:, :7].view(np.int32)).to(self.device)
        else:
            before[:, :7] = rec[:, :7]   # the board before the move, the mover's indicator (bgx/records.py)
        obs = ops.encode_packed(before)
        rewards = rec[:, 9].contiguous().view(torch.float32)
        wins = [WIN_TYPES[int(w) & 0xFF] for w in (hdr[:, 5] & 0xFF).tolist()]
        return obs, rewards, lens.tolist(), wins, self._record_movers(rec)

    @staticmethod
    def _record_movers(rec):
        """int32 [m]: the mover of each record, word 11 bit 9 (bgx/records.py)."""
        return (rec[:, 11] >> 9) & 1

    @staticmethod
    def _observation_movers(obs):
        """int32 [m]: feature 197, the indicator of player 1 (the mover in engine records)."""
        return (obs[:, 197] != 0).to(torch.int32)

    def _from_episodes(self, episodes):
        obs, rew, lens, wins = [], [], [], []
        for ep in episodes:
            obs.extend(torch.as_tensor(np.asarray(x.observation, np.float32)) for x in ep.experiences)
            rew.extend(float(np.asarray(x.reward)) for x in ep.experiences)
            lens.append(len(ep.experiences))
            wins.append(ep.win_type)
        obs_t = torch.stack(obs).to(self.device) if obs else torch.zeros((0, 198), device=self.device)
        movers = self._observation_movers(obs_t)
        if self.afterstates and obs:   # next_observation under the mover's indicator, not the next player's
            nxt = [torch.as_tensor(np.asarray(x.next_observation, np.float32)) for ep in episodes for x in ep.experiences]
            obs_t = torch.stack(nxt).to(self.device)
            obs_t[:, 196] = (movers == 0).to(obs_t.dtype)
            obs_t[:, 197] = (movers == 1).to(obs_t.dtype)
        return obs_t, torch.tensor(rew, dtype=torch.float32, device=self.device), lens, wins, movers

    # ------------------------------------------------------------ update
    def update(self, episodes):
        """Trainer.update(episodes) (trainer.py:49-166): exactly batch_episode_size episodes."""
        if len(episodes) != self.batch_episode_size:
            raise ValueError(f"Expected {self.batch_episode_size} episodes, but got {len(episodes)}.")
        return self._update(*self._from_episodes(episodes))

    def update_records(self, headers, records):
        """The same update from compact records (headers [n, 16], records [m, 12],
        each episode's records contiguous in header order); any n >= 1."""
        if self.backend == "hip":
            if self.lam != 0.0 and not self.batched:
                raise ValueError("the sequential HIP update (bgx_td0_update) is TD(0) only: for lam != 0 use "
                                 "batched=True with backend='hip', or backend='torch'")
            if self.zero_sum and not self.batched:
                raise ValueError("the sequential HIP update (bgx_td0_update) keeps the reference's TD(0) target: for "
                                 "zero_sum=True use batched=True with backend='hip', or backend='torch'")
            if self.afterstates and not self.batched:
                raise ValueError("the sequential HIP update (bgx_td0_update) keeps the reference's before-move "
                                 "positions: for afterstates=True use batched=True with backend='hip', or "
                                 "backend='torch'")
            return self._update_hip_batched(headers, records) if self.batched else self._update_hip(headers, records)
        return self._update(*self._from_records(headers, records))

    # ------------------------------------------------------------ HIP backend
    _KEYS = ("fc1.weight", "fc1.bias", "value_head.weight", "value_head.bias")

    def _hip_state(self):
        """Flat fp32 params / Adam moments (state_dict order) and the step count,
        taken over from the torch module / optimizer the first time."""
        if self._flat is not None and self._flat.get("token") != self._module_token():
            self._flat = None   # the module / optimizer changed outside the HIP updates: take it over again
        if self._flat is None:
            net, opt = self.policy_network, self.optimizer
            params = [dict(net.named_parameters())[k] for k in self._KEYS]
            flat = torch.cat([p.detach().reshape(-1) for p in params]).contiguous()
            m = torch.zeros_like(flat)
            v = torch.zeros_like(flat)
            step = 0
            st = [opt.state.get(p, {}) for p in params]
            if all("exp_avg" in x for x in st):
                m = torch.cat([x["exp_avg"].reshape(-1) for x in st]).contiguous()
                v = torch.cat([x["exp_avg_sq"].reshape(-1) for x in st]).contiguous()
                step = int(float(st[0]["step"]))
            self._flat = {"p": flat, "m": m, "v": v,
                          "step": torch.tensor([step], dtype=torch.int32, device=self.device),
                          "token": self._module_token()}
        return self._flat

    def _module_token(self):
        """Identifies the module's parameters and the optimizer's moments as the
        HIP backend last left them: every in-place write (load_state_dict,
        copy_, an optimizer step) bumps a tensor's _version, and replacing the
        optimizer state swaps the moment tensors."""
        net, opt = self.policy_network, self.optimizer
        params = [dict(net.named_parameters())[k] for k in self._KEYS]
        st = [opt.state.get(p, {}) for p in params]
        return (tuple(p._version for p in params),
                tuple((id(x.get("exp_avg")), id(x.get("exp_avg_sq")), id(x.get("step"))) for x in st))

    def _sync_module(self):
        """Copy the HIP backend's weights / moments back into the torch module and
        optimizer (state_dict consumers, and a later torch-backend update)."""
        f = self._flat
        net, opt = self.policy_network, self.optimizer
        params = [dict(net.named_parameters())[k] for k in self._KEYS]
        o = 0
        step = int(f["step"].item())
        with torch.no_grad():
            for p in params:
                n = p.numel()
                p.copy_(f["p"][o:o + n].view_as(p))
                if step > 0:
                    st = opt.state[p]
                    st["exp_avg"] = f["m"][o:o + n].view_as(p).clone()
                    st["exp_avg_sq"] = f["v"][o:o + n].view_as(p).clone()
                    st["step"] = torch.tensor(float(step))
                o += n
        f["token"] = self._module_token()

    def _update_hip(self, headers, records):
        rec, hdr, lens, offs_h = self._host_inputs(headers, records)
        if len(lens) and int(lens.max()) > 2048:
            raise ValueError("bgx_td0_update: an episode has more than 2048 records")
        if len(lens) and int(lens.min()) <= 0:
            # the kernel skips an empty episode (no Adam step), while the metrics
            # below divide by every episode: reject it instead of skewing them
            raise ValueError("bgx_td0_update: an episode has no records")
        n_rec = int(rec.shape[0])
        if int(offs_h[-1]) != n_rec or n_rec >= 2 ** 31:
            # the kernel reads records [0, offs[-1]): fewer than that would be read past the tensor's end
            raise ValueError(f"bgx_td0_update: the headers count {int(offs_h[-1])} records, got {n_rec}")
        from ._lib import check, lib, ptr, stream_handle
        offs = torch.as_tensor(offs_h.astype(np.int32), device=self.device)
        f = self._hip_state()
        metrics = torch.zeros(5, dtype=torch.float64, device=self.device)
        n_eps = len(lens)
        clip = float(self.grad_clip) if self.grad_clip is not None else 0.0
        with torch.cuda.device(self.device):   # the trainer's device and its current stream
            check(lib().bgx_td0_update(ptr(rec), ptr(offs), n_eps, ptr(f["p"]), ptr(f["m"]), ptr(f["v"]),
                                       ptr(f["step"]), float(self.optimizer.param_groups[0]["lr"]),
                                       float(self.gamma), clip, ptr(metrics),
                                       stream_handle(torch.cuda.current_stream(self.device))),
                  "bgx_td0_update")
        return self._finish_hip(metrics, hdr, lens)

    def _update_hip_batched(self, headers, records):
        """One call of the batched update (the entry point ops.td_batched_entry
        picks for lam / zero_sum / afterstates): one Adam step on the mean of
        the per-episode losses (the torch batched path's semantics)."""
        rec, hdr, lens, offs_h = self._host_inputs(headers, records)
        n_eps, n_rec = len(lens), int(rec.shape[0])
        if n_eps < 1:
            raise ValueError("bgx_td0_update_batched: no episodes")
        if int(lens.min()) <= 0:
            raise ValueError("bgx_td0_update_batched: an episode has no records")
        if (np.diff(offs_h) < 1).any() or int(offs_h[-1]) != n_rec or n_rec >= 2 ** 31:
            raise ValueError(f"bgx_td0_update_batched: the headers count {int(offs_h[-1])} records, got {n_rec}")
        offs = torch.as_tensor(offs_h.astype(np.int32), device=self.device)
        f = self._hip_state()
        entry, flags = ops.td_batched_entry(self.lam, self.zero_sum, self.afterstates)
        need = ops.td_batched_workspace(entry, n_rec)
        if self._work is None or self._work.numel() < need or self._work.device != f["p"].device:
            self._work = torch.empty(need, dtype=torch.uint8, device=self.device)
        metrics = torch.zeros(5, dtype=torch.float64, device=self.device)
        d_hdr = torch.from_numpy(np.ascontiguousarray(hdr).view(np.int32)).to(self.device) if self.afterstates else None
        with torch.cuda.device(self.device):   # the trainer's device and its current stream
            ops.td_batched(entry, records=rec, headers=d_hdr, offs=offs, n_eps=n_eps, n_rec=n_rec,
                           state=(f["p"], f["m"], f["v"], f["step"]), lr=float(self.optimizer.param_groups[0]["lr"]),
                           gamma=float(self.gamma), lam=self.lam, flags=flags,
                           clip=float(self.grad_clip) if self.grad_clip is not None else 0.0, metrics=metrics,
                           work=self._work, stream=torch.cuda.current_stream(self.device))
        return self._finish_hip(metrics, hdr, lens)

    # ------------------------------------------------------------ device-resident update
    def update_device(self, headers, records, offs=None):
        """update_records for a learner that keeps everything on the device
        (bgx/learner.py): `headers` int32 [n, 16] and `records` int32 [m, 12] are
        contiguous device tensors, e.g. a harvest ticket's own arrays
        (Engine.harvest_fetch(clone=False)). Needs batched=True and
        backend="hip". No tensor is read on the host: the offsets come from
        ops.episode_offsets, n and m from the shapes, the ABI call is the one
        _update_hip_batched makes (the headers go in as d_headers), and the
        five metrics add up in a device tensor the trainer owns. The torch
        module, the optimizer and the parameter manager are not touched:
        metrics(), sync_module(), state_dict() and publish() bring the host up
        to date when asked. On the same inputs and state the flat parameters,
        moments and step count come out bit-identical to update_records'.

        What update_records checks on the host (every episode has records, the
        headers count exactly m records) cannot be checked here without a
        round trip: the headers are trusted as the engine wrote them, and the
        kernels clamp the offsets to [0, m] (no read past `records`).
        offs: the headers' episode offsets where the caller has them already
        (int32 [n + 1] on the device, e.g. ops.canonical_harvest's): the
        offsets launch is then left out.
        Returns None; asynchronous on the trainer's current stream."""
        if not (self.batched and self.backend == "hip"):
            raise ValueError("update_device needs batched=True and backend='hip' (the batched HIP update is the only "
                             "one that runs without the host)")
        for name, t, width in (("headers", headers, 16), ("records", records, 12)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int32 or t.dim() != 2 \
                    or t.shape[1] != width or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous int32 device tensor [n, {width}]")
            if t.device != self.device and not (self.device.index is None and t.device.type == "cuda"):
                raise ValueError(f"{name} are on {t.device}, the trainer on {self.device}")
        n_eps, n_rec = int(headers.shape[0]), int(records.shape[0])
        if n_eps < 1:
            raise ValueError("update_device: no episodes")
        if n_rec < n_eps or n_rec >= 2 ** 31:
            raise ValueError(f"update_device: {n_eps} episodes cannot hold {n_rec} records")
        if offs is not None and (not isinstance(offs, torch.Tensor) or offs.dtype != torch.int32 or offs.dim() != 1
                                 or offs.numel() != n_eps + 1 or offs.device != headers.device
                                 or not offs.is_contiguous()):
            raise ValueError("offs must be a contiguous int32 [n + 1] tensor on the headers' device")
        f = self._hip_state()
        dev = f["p"].device
        if self._dev is None or self._dev["metrics"].device != dev:
            self._dev = {"metrics": torch.zeros(5, dtype=torch.float64, device=dev), "offs": None,
                         "updates": 0, "episodes": 0, "records": 0}
        d = self._dev
        entry, flags = ops.td_batched_entry(self.lam, self.zero_sum, self.afterstates)
        need = ops.td_batched_workspace(entry, n_rec)
        # both buffers grow in steps, so a steady state allocates nothing
        if self._work is None or self._work.numel() < need or self._work.device != dev:
            self._work = torch.empty(need + need // 4, dtype=torch.uint8, device=dev)
        if offs is None and (d["offs"] is None or d["offs"].numel() < n_eps + 1):
            d["offs"] = torch.empty(2 * (n_eps + 1), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):   # the trainer's device and its current stream
            s = torch.cuda.current_stream(dev)
            if offs is None:
                offs = ops.episode_offsets(headers, out=d["offs"], stream=s)
            ops.td_batched(entry, records=records, headers=headers, offs=offs, n_eps=n_eps, n_rec=n_rec,
                           state=(f["p"], f["m"], f["v"], f["step"]), lr=float(self.optimizer.param_groups[0]["lr"]),
                           gamma=self._gamma_host, lam=self.lam, flags=flags,
                           clip=float(self.grad_clip) if self.grad_clip is not None else 0.0, metrics=d["metrics"],
                           work=self._work, stream=s)
        d["updates"] += 1
        d["episodes"] += n_eps
        d["records"] += n_rec
        self.total_episodes += n_eps

    @property
    def params(self):
        """The flat float32 [25601] device parameters (state_dict order) the HIP
        updates write in place: what Engine.set_weights_device takes."""
        return self._hip_state()["p"]

    def metrics(self, reset=True):
        """update_records' metrics dict over the update_device calls since the
        last reset, each value a mean per episode (one host read of the device
        accumulator); None when there were none. No win_counts: those would
        need the headers on the host."""
        d = self._dev
        if d is None or d["updates"] == 0:
            return None
        a = d["metrics"].tolist()
        n = max(1, d["episodes"])
        out = {"loss": a[0] / n, "grad_norm": a[1] / n, "td_error": a[2] / n, "predicted_value": a[3] / n,
               "reward": a[4] / n, "episode_length": float(d["records"]) / n, "episodes": d["episodes"],
               "updates": d["updates"]}
        if reset:
            d["metrics"].zero_()
            d["updates"] = d["episodes"] = d["records"] = 0
        return out

    def sync_module(self):
        """The torch module and optimizer follow the HIP backend's flat state
        (update_device leaves them behind)."""
        if self._flat is not None:
            self._sync_module()

    def state_dict(self):
        """The current weights as the module's state_dict, after sync_module()."""
        self.sync_module()
        return self.policy_network.state_dict()

    def publish(self):
        """The current weights to the parameter manager (what every
        update_records call does; update_device leaves it to the caller)."""
        self.parameter_manager.set_parameters(self.state_dict())

    def _finish_hip(self, metrics, hdr, lens):
        """After a HIP update: the module / optimizer follow the flat state, the
        weights go to the parameter manager, the device metrics become the dict."""
        n_eps = len(lens)
        self.total_episodes += n_eps
        self._sync_module()
        a = metrics.tolist()
        win_counts = {"regular": 0, "gammon": 0, "backgammon": 0}
        for w in (hdr[:, 5] & 0xFF).tolist():
            name = WIN_TYPES[int(w)]
            if name in win_counts:
                win_counts[name] += 1
        self.parameter_manager.set_parameters(self.policy_network.state_dict())
        out = {"loss": a[0], "grad_norm": a[1], "td_error": a[2], "predicted_value": a[3], "reward": a[4],
               "episode_length": float(lens.sum())}
        out = {k: v / max(1, n_eps) for k, v in out.items()}
        out["win_counts"] = win_counts
        out["episodes"] = n_eps
        return out

    def _update(self, obs, rewards, lens, wins, movers=None):
        if self._flat is not None:   # continue from the HIP backend's state
            self._sync_module()
            self._flat = None
        net, opt = self.policy_network, self.optimizer
        params = list(net.parameters())
        n_eps = len(lens)
        self.total_episodes += n_eps
        m = {"loss": 0.0, "td_error": 0.0, "grad_norm": 0.0, "predicted_value": 0.0, "reward": 0.0,
             "episode_length": 0.0}
        win_counts = {"regular": 0, "gammon": 0, "backgammon": 0}
        offs = np.concatenate([[0], np.cumsum(lens)]).tolist()
        # metrics accumulate on the device; one host read per update
        acc = torch.zeros(6, dtype=torch.float64, device=self.device)
        if self.batched:
            losses, ys, tgts = [], [], []
            for e in range(n_eps):
                y, tgt = self._episode_terms(obs, rewards, offs[e], offs[e + 1], movers)
                losses.append(F.mse_loss(y, tgt))
                ys.append(y.detach().reshape(-1))
                tgts.append(tgt.reshape(-1))
            opt.zero_grad()
            loss = torch.stack(losses).mean()
            loss.backward()
            if self.grad_clip is not None and self.grad_clip > 0:   # <= 0: no clipping, as the HIP backend reads it
                pre = torch.nn.utils.clip_grad_norm_(params, self.grad_clip)
                post = pre * torch.clamp(self.grad_clip / (pre + 1e-6), max=1.0)
            else:
                post = torch.norm(torch.stack([p.grad.detach().norm(2) for p in params if p.grad is not None]), 2)
            opt.step()
            # the sequential path's metrics, summed over the episodes (the one norm counts for each)
            yd, tg = torch.cat(ys).double(), torch.cat(tgts).double()
            inv_t = 1.0 / torch.as_tensor(np.repeat(lens, lens), device=self.device).double()
            acc[0] = loss.detach() * n_eps
            acc[1] = post.double() * n_eps
            acc[2] = ((tg - yd).abs() * inv_t).sum()
            acc[3] = (yd * inv_t).sum()
            acc[4] = rewards[:offs[-1]].sum().double()
        else:
            for e in range(n_eps):
                y, tgt = self._episode_terms(obs, rewards, offs[e], offs[e + 1], movers)
                loss = F.mse_loss(y, tgt)
                opt.zero_grad()
                loss.backward()
                if self.grad_clip is not None:
                    pre = torch.nn.utils.clip_grad_norm_(params, self.grad_clip)
                    # the reference measures the norm after clipping (trainer.py:130-135):
                    # torch scales by min(1, clip / (norm + 1e-6))
                    post = pre * torch.clamp(self.grad_clip / (pre + 1e-6), max=1.0)
                else:
                    post = torch.norm(torch.stack([p.grad.detach().norm(2) for p in params if p.grad is not None]), 2)
                opt.step()
                yd = y.detach()
                acc += torch.stack([loss.detach().double(), post.double(), (tgt - yd).abs().mean().double(),
                                    yd.mean().double(), rewards[offs[e]:offs[e + 1]].sum().double(),
                                    torch.zeros((), dtype=torch.float64, device=self.device)])
        a = acc.tolist()
        m["loss"], m["grad_norm"], m["td_error"], m["predicted_value"], m["reward"] = a[0], a[1], a[2], a[3], a[4]
        m["episode_length"] = float(offs[-1])
        for w in wins:
            if w in win_counts:
                win_counts[w] += 1
        self.parameter_manager.set_parameters(net.state_dict())
        out = {k: v / max(1, n_eps) for k, v in m.items()}
        out["win_counts"] = win_counts
        out["episodes"] = n_eps
        return out

    def _episode_terms(self, obs, rewards, a, b, movers=None):
        """(Y with its graph, the detached target) of the episode of records a .. b-1;
        movers [m]: every record's mover, read when zero_sum is set."""
        y = self.policy_network(obs[a:b]).squeeze()
        tgt = rewards[a:b].clone().squeeze()
        if self.zero_sum and movers is None:
            raise ValueError("zero_sum=True needs the records' movers")
        if self.lam != 0.0 or self.zero_sum:
            if b - a > 1:   # the serial recurrence in y's dtype, from the episode's end
                from .train_ref import lambda_returns
                mv = movers[a:b].cpu().numpy() if self.zero_sum else None
                g = lambda_returns(y.detach().reshape(-1).cpu().numpy(), rewards[a:b].cpu().numpy(), [0, b - a],
                                   float(self.gamma), self.lam, movers=mv)
                tgt = torch.from_numpy(g).to(y.device)
        elif b - a > 1:
            tgt[:-1] += self.gamma * y[1:].detach()
        return y, tgt
