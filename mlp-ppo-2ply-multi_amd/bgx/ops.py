"""Stateless device ops over libbgx.so (the parity entry points of include/bgx.h).

Each op mirrors one reference function on a batch of boards:
  movegen      get_all_possible_moves + execute_full_move_on_board_copy
               (backgammon/moves/generate_all_moves.py:7-90, environments/env_helper.py:27-91)
  encode       ImmutableBoard.get_board_features (board/immutable_board.py:86-128),
               layout=1: generate_board_tensor.compute_features (:98-140)
  Net.value    BackgammonPolicyNetwork.forward (agents/policy_network.py:53-70)
Boards are uint8 [n, 52] device tensors in the reference's field order.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ._lib import check, lib, ptr, require_cuda, stream_handle


def _u8(t, shape_last=None):
    t = torch.as_tensor(t)
    if t.dtype != torch.uint8:
        t = t.to(torch.uint8)
    if not t.is_cuda:
        t = t.cuda()
    return t.contiguous()


def movegen(boards, player, dice, cap: int = 512, stream=None):
    """Ordered result boards for n (board, player, dice) jobs.

    Returns (out uint8 [n, cap, 52], count int32 [n]); count is the full
    number of results, rows k >= min(count, cap) are unspecified."""
    boards, player, dice = _u8(boards).view(-1, 52), _u8(player).view(-1), _u8(dice).view(-1, 2)
    n = boards.shape[0]
    require_cuda(boards, player, dice)
    out = torch.empty((n, cap, 52), dtype=torch.uint8, device=boards.device)
    cnt = torch.empty((n,), dtype=torch.int32, device=boards.device)
    check(lib().bgx_movegen(ptr(boards), ptr(player), ptr(dice), n, ptr(out), ptr(cnt), cap,
                            stream_handle(stream)), "bgx_movegen")
    return out, cnt


BAD_BITS = {1: "a point held by both players", 2: "more than 15 checkers of a player",
            4: "a count above 15", 8: "a die outside 1..6", 16: "a player not 0/1"}


def check_boards(boards, player=None, dice=None, stream=None):
    """The input-domain check of the stateless ops (include/bgx.h BGX_BADF_*)
    on the device: returns (flags, first bad index or -1)."""
    boards = _u8(boards).view(-1, 52)
    require_cuda(boards)
    player = None if player is None else _u8(player).view(-1)
    dice = None if dice is None else _u8(dice).view(-1, 2)
    f, first = ctypes.c_uint32(0), ctypes.c_int32(-1)
    check(lib().bgx_check_boards(ptr(boards), ptr(player), ptr(dice), boards.shape[0], ctypes.byref(f),
                                 ctypes.byref(first), stream_handle(stream)), "bgx_check_boards")
    return int(f.value), int(first.value)


def encode(boards, player, layout: int = 0, stream=None):
    boards, player = _u8(boards).view(-1, 52), _u8(player).view(-1)
    require_cuda(boards, player)
    n = boards.shape[0]
    out = torch.empty((n, 198), dtype=torch.float32, device=boards.device)
    check(lib().bgx_encode(ptr(boards), ptr(player), n, ptr(out), int(layout), stream_handle(stream)),
          "bgx_encode")
    return out


def encode_packed(packed, layout: int = 0, stream=None):
    """encode() of the engine's own packed boards (int32 [n, 8]: harvest
    records / headers, the indicator in word 6): no input-domain check and no
    synchronization (bgx_encode_packed; such boards come from the engine)."""
    packed = torch.as_tensor(packed)
    if not packed.is_cuda:
        packed = packed.cuda()
    packed = packed.contiguous().view(-1, 8)
    require_cuda(packed)
    n = packed.shape[0]
    out = torch.empty((n, 198), dtype=torch.float32, device=packed.device)
    check(lib().bgx_encode_packed(ptr(packed), n, ptr(out), int(layout), stream_handle(stream)),
          "bgx_encode_packed")
    return out


def reply_moves(boards, opponent, cap: int = 0, stream=None):
    """The 2-ply reply expansion (include/bgx.h bgx_reply_moves): for each
    candidate board, the opponent's afterstates for the 21 DICE_ROLLS.
    Returns (rows int32 [cap, 8] packed, off int32 [n * 21], cnt int32 [n * 21])."""
    boards, opponent = _u8(boards).view(-1, 52), _u8(opponent).view(-1)
    require_cuda(boards, opponent)
    n = boards.shape[0]
    # records (<= 64 per (board, roll) on average, generously) + per workgroup
    # of the launch (two per CU, at most ceil(7 n / 16): bgx_launch_movegen) two
    # row chunks' worth (2 x 2,048 rows: its last chunk's tail and its waves'
    # kept remainders, each smaller than one request); running out is an error
    # (BGX_E_CAPACITY), never a silent truncation
    n_cu = torch.cuda.get_device_properties(boards.device).multi_processor_count
    cap = cap or n * 21 * 64 + min(2 * n_cu, (n * 7 + 15) // 16) * 2 * 2048 + 4096
    out = torch.empty((cap, 8), dtype=torch.int32, device=boards.device)
    off = torch.empty((n * 21,), dtype=torch.int32, device=boards.device)
    cnt = torch.empty((n * 21,), dtype=torch.int32, device=boards.device)
    check(lib().bgx_reply_moves(ptr(boards), ptr(opponent), n, ptr(out), cap, ptr(off), ptr(cnt),
                                stream_handle(stream)), "bgx_reply_moves")
    return out, off, cnt


def pack(boards, player, stream=None):
    boards, player = _u8(boards).view(-1, 52), _u8(player).view(-1)
    require_cuda(boards, player)
    n = boards.shape[0]
    out = torch.empty((n, 8), dtype=torch.int32, device=boards.device)
    check(lib().bgx_pack(ptr(boards), ptr(player), n, ptr(out), stream_handle(stream)), "bgx_pack")
    return out


def unpack(packed, stream=None):
    """Packed boards (int32 [n, 8]) -> uint8 [n, 52]; the indicator player is
    bits 16.. of word 6."""
    packed = torch.as_tensor(packed).contiguous()
    require_cuda(packed)
    n = packed.shape[0]
    out = torch.empty((n, 52), dtype=torch.uint8, device=packed.device)
    check(lib().bgx_unpack(ptr(packed), n, ptr(out), stream_handle(stream)), "bgx_unpack")
    return out


def packed_player(packed):
    return ((packed[:, 6] >> 16) & 1).to(torch.uint8)


def weights_from(obj):
    """Host fp32 (W1 [128,198], b1 [128], w2 [128], b2 [1]) from a state_dict
    (fc1.weight, fc1.bias, value_head.weight, value_head.bias) or a dict with
    keys W1, b1, w2, b2."""
    if "fc1.weight" in obj:
        W1, b1 = obj["fc1.weight"], obj["fc1.bias"]
        w2, b2 = obj["value_head.weight"], obj["value_head.bias"]
    else:
        W1, b1, w2, b2 = obj["W1"], obj["b1"], obj["w2"], obj["b2"]

    def f(x, shape):
        if isinstance(x, torch.Tensor):
            x = x.detach().float().cpu().numpy()
        return np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(shape))

    W1 = f(W1, (128, 198))
    if W1.shape != (128, 198):
        raise ValueError("fc1.weight must be [128, 198] (BackgammonPolicyNetwork hidden_size=128)")
    return W1, f(b1, (128,)), f(w2, (128,)), f(b2, (1,))


def _fp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Net:
    """Device copy of BackgammonPolicyNetwork weights (fp32 + split-fp16 MFMA fragments).
    Raises BgxError (BGX_E_ARG) for a non-finite weight or max|log2(e) w| >= 2^26
    over W1 / b1 (include/bgx.h, bgx_net_create)."""

    def __init__(self, weights):
        W1, b1, w2, b2 = weights_from(weights)
        if not torch.cuda.is_available():
            require_cuda()
        h = ctypes.c_void_p()
        check(lib().bgx_net_create(_fp(W1), _fp(b1), _fp(w2), _fp(b2), ctypes.byref(h)),
              "bgx_net_create")
        self._h = h
        self._destroy = lib().bgx_net_destroy   # bound now: module globals are gone at interpreter exit

    def __del__(self):
        h = getattr(self, "_h", None)
        destroy = getattr(self, "_destroy", None)
        if h and h.value and destroy is not None:
            destroy(h)
            self._h = None

    def value(self, x, stream=None):
        """V for fp32 features [n, 198] (generic fp32 FMA path)."""
        x = torch.as_tensor(x, dtype=torch.float32)
        if not x.is_cuda:
            x = x.cuda()
        x = x.contiguous().view(-1, 198)
        out = torch.empty((x.shape[0],), dtype=torch.float32, device=x.device)
        check(lib().bgx_value(self._h, ptr(x), x.shape[0], ptr(out), stream_handle(stream)), "bgx_value")
        return out

    def value_boards(self, boards, player, stream=None):
        """V of get_board_features(board, player) via the fused split-fp16 MFMA kernel."""
        boards, player = _u8(boards).view(-1, 52), _u8(player).view(-1)
        require_cuda(boards, player)
        out = torch.empty((boards.shape[0],), dtype=torch.float32, device=boards.device)
        check(lib().bgx_value_boards(self._h, ptr(boards), ptr(player), boards.shape[0], ptr(out),
                                     stream_handle(stream)), "bgx_value_boards")
        return out

    def two_ply(self, boards, opponent, sample=0, seed=0, stream=None):
        """compute_weighted_opponent_response (two_ply.py:93-150) for afterstates
        [n, 52]; returns float64 W [n]. sample=0: exact mode; sample=50: the
        reference's random.sample of 50 replies for 1-1 / 2-2 / 3-3
        (two_ply.py:119-121), reproducible per seed."""
        boards, opponent = _u8(boards).view(-1, 52), _u8(opponent).view(-1)
        require_cuda(boards, opponent)
        out = torch.empty((boards.shape[0],), dtype=torch.float64, device=boards.device)
        check(lib().bgx_two_ply_sampled(self._h, ptr(boards), ptr(opponent), boards.shape[0], int(sample),
                                        int(seed), ptr(out), stream_handle(stream)), "bgx_two_ply_sampled")
        return out


def value_boards_routed(net0, net1, boards, player, net_id, stream=None):
    """value_boards with a network per board (bgx_value_boards_routed): net_id
    uint8 [n] in {0, 1} picks net0 or net1 (two Net objects) for each board.
    The match mode's routed MFMA launch; each V has the bits
    Net.value_boards gives under the board's own network."""
    boards, player, net_id = _u8(boards).view(-1, 52), _u8(player).view(-1), _u8(net_id).view(-1)
    require_cuda(boards, player, net_id)
    if net_id.shape[0] != boards.shape[0]:
        raise ValueError("net_id must hold one entry per board")
    out = torch.empty((boards.shape[0],), dtype=torch.float32, device=boards.device)
    check(lib().bgx_value_boards_routed(net0._h, net1._h, ptr(boards), ptr(player), ptr(net_id), boards.shape[0],
                                        ptr(out), stream_handle(stream)), "bgx_value_boards_routed")
    return out


def rollout_tally(headers, start_player, n_pos, max_episode, counts, stream=None):
    """counts[pos][8] += the results of `headers` (bgx_rollout_tally; bgx/rollout.py
    tally_counts is its numpy statement): headers int32 [n, 16] on the device (a
    harvest's), start_player uint8 [n_pos] and counts int64 [n_pos, 8] (the bits
    of the u64 counters) on the same device. Asynchronous on the stream; the
    caller zeroes counts once, calls accumulate. Returns counts."""
    require_cuda(headers, start_player, counts)   # device tensors, contiguous
    if not (headers.device == start_player.device == counts.device):
        raise ValueError("headers, start_player and counts must be on the same device")
    n_pos = int(n_pos)
    if headers.dtype != torch.int32 or headers.dim() != 2 or headers.shape[1] != 16:
        raise ValueError("headers must be int32 [n, 16]")
    if start_player.dtype != torch.uint8 or start_player.numel() != n_pos:
        raise ValueError("start_player must be uint8 [n_pos]")
    if counts.dtype != torch.int64 or counts.numel() != n_pos * 8:
        raise ValueError("counts must be int64 [n_pos, 8]")
    check(lib().bgx_rollout_tally(ptr(headers), int(headers.shape[0]), ptr(start_player), n_pos, int(max_episode),
                                  ptr(counts), stream_handle(stream)), "bgx_rollout_tally")
    return counts


def episode_offsets(headers, out=None, stream=None):
    """offs int32 [n + 1] of a harvest's headers (int32 [n, 16] on the device),
    computed there (bgx_episode_offsets): offs[0] = 0, offs[k + 1] = offs[k] +
    headers[k, 3]. Asynchronous on the stream; nothing is read on the host. `out`:
    a device int32 tensor of at least n + 1 elements to write into (no allocation
    then); the result is its first n + 1 elements."""
    require_cuda(headers)
    if headers.dtype != torch.int32 or headers.dim() != 2 or headers.shape[1] != 16:
        raise ValueError("headers must be int32 [n, 16]")
    n = int(headers.shape[0])
    if out is None:
        out = torch.empty((n + 1,), dtype=torch.int32, device=headers.device)
    else:
        require_cuda(out)
        if out.dtype != torch.int32 or out.dim() != 1 or out.numel() < n + 1 or out.device != headers.device:
            raise ValueError("out must be int32 [>= n + 1] on the headers' device")
    with torch.cuda.device(headers.device):
        check(lib().bgx_episode_offsets(ptr(headers), n, ptr(out), stream_handle(stream)), "bgx_episode_offsets")
    return out[:n + 1]


TDF_ZERO_SUM = 1   # BGX_TDF_ZERO_SUM (include/bgx.h)

# The batched TD update's entry points (include/bgx.h): each one's workspace
# query, and which of headers / lam / flags / target_out its signature has
# beside the arguments all four share.
TD_BATCHED = {
    "bgx_td0_update_batched": ("bgx_td0_batch_workspace", ()),
    "bgx_tdlambda_update_batched": ("bgx_tdlambda_batch_workspace", ("lam", "target_out")),
    "bgx_td_update_batched": ("bgx_tdlambda_batch_workspace", ("lam", "flags", "target_out")),
    "bgx_td_afterstate_update_batched": ("bgx_td_afterstate_batch_workspace",
                                         ("headers", "lam", "flags", "target_out")),
}


def td_batched_entry(lam=0.0, zero_sum=False, afterstates=False):
    """(entry name, flags) of the batched update that serves a trainer's options:
    the afterstate entry, else bgx_td_update_batched when zero_sum, else
    bgx_tdlambda_update_batched when lam != 0, else bgx_td0_update_batched (one
    launch fewer and no targets in its workspace)."""
    flags = TDF_ZERO_SUM if zero_sum else 0
    if afterstates:
        return "bgx_td_afterstate_update_batched", flags
    if zero_sum:
        return "bgx_td_update_batched", flags
    return ("bgx_tdlambda_update_batched" if lam != 0.0 else "bgx_td0_update_batched"), 0


def td_batched_workspace(entry, n_rec):
    """Bytes of workspace `entry` needs for n_rec records (host arithmetic)."""
    query = TD_BATCHED[entry][0]
    need = ctypes.c_uint64(0)
    check(getattr(lib(), query)(int(n_rec), ctypes.byref(need)), query)
    return int(need.value)


def td_batched_call(entry, *, records, offs, n_eps, n_rec, state, lr, gamma, clip, metrics, work, work_bytes=None,
                    headers=None, lam=0.0, flags=0, grad_out=None, target_out=None, stream=None):
    """One call of a batched-update entry point, its named arguments laid out in
    that entry's positional order; returns the code (td_batched: raises on one).
    Tensors are contiguous device tensors or None (a null pointer); state = the
    flat (params, Adam m, Adam v, step). headers, lam, flags and target_out go
    only to the entries that have them; work_bytes defaults to all of `work`.
    Asynchronous on the stream (default: the current one)."""
    has = TD_BATCHED[entry][1]
    p, m, v, step = state
    args = [ptr(records)] + ([ptr(headers)] if "headers" in has else []) + \
           [ptr(offs), int(n_eps), int(n_rec), ptr(p), ptr(m), ptr(v), ptr(step), lr, gamma] + \
           ([lam] if "lam" in has else []) + ([int(flags)] if "flags" in has else []) + \
           [clip, ptr(metrics), ptr(grad_out)] + ([ptr(target_out)] if "target_out" in has else []) + \
           [ptr(work), work.numel() if work_bytes is None else int(work_bytes), stream_handle(stream)]
    return getattr(lib(), entry)(*args)


def td_batched(entry, **kw):
    check(td_batched_call(entry, **kw), entry)


CANON_BITS = {1: "a lane outside [lane_base, lane_base + lanes)", 2: "two episodes share (lane, episode number)",
              4: "the headers' record counts do not sum to the records given"}


def canonical_workspace(n_eps, lanes):
    """Bytes of workspace canonical_harvest needs (bgx_harvest_canonical_workspace; host arithmetic)."""
    need = ctypes.c_uint64(0)
    check(lib().bgx_harvest_canonical_workspace(int(n_eps), int(lanes), ctypes.byref(need)),
          "bgx_harvest_canonical_workspace")
    return int(need.value)


def canonical_harvest(headers, records, lane_base=0, lanes=None, out=None, status=None, stream=None, work=None):
    """A harvest in canonical order, computed on the device (bgx_harvest_canonical):
    the episodes of `headers` int32 [n, 16] / `records` int32 [m, 12] (contiguous
    device tensors, e.g. a ticket's own arrays) ordered by (lane, episode number),
    header words 0 and 1 as unsigned. Returns (headers [n, 16], records [m, 12],
    offs int32 [n + 1]): the headers and each episode's records verbatim in that
    order and episode_offsets of the new headers. Any arrival order of the same
    episodes gives the same bytes. Asynchronous on the stream.

    lane_base, lanes: the range of header word 0 (an Engine's lane_base and
    lanes). lanes=None reads the largest lane from the headers on the host, which
    waits for them; pass it to keep the call asynchronous.
    out: three device tensors to write into, int32 [>= n, 16], [>= m, 12] and
    [>= n + 1]; the results are views of their first rows. status: an int32 [1]
    device tensor the call ORs CANON_BITS into and never clears (zero after a
    harvest as the engine writes it; with a bit set the outputs are unspecified).
    work: a uint8 device tensor of at least bgx_harvest_canonical_workspace
    bytes. What is not given is allocated on the stream."""
    for name, t, width in (("headers", headers, 16), ("records", records, 12)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int32 or t.dim() != 2 \
                or t.shape[1] != width or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous int32 device tensor [n, {width}]")
    dev = headers.device
    if records.device != dev:
        raise ValueError(f"headers are on {dev}, records on {records.device}")
    n, m = int(headers.shape[0]), int(records.shape[0])
    if m >= 2 ** 31:
        raise ValueError(f"canonical_harvest: {m} records")
    lane_base = int(lane_base)
    if lanes is None:
        lanes = max(1, int(headers[:, 0].max()) - lane_base + 1) if n else 1
    lanes = int(lanes)
    if lane_base < 0 or lanes < 1:
        raise ValueError(f"canonical_harvest: lane_base={lane_base} lanes={lanes}")
    need = canonical_workspace(n, lanes)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(s):
        if out is None:
            out = (torch.empty((n, 16), dtype=torch.int32, device=dev), torch.empty((m, 12), dtype=torch.int32, device=dev),
                   torch.empty((n + 1,), dtype=torch.int32, device=dev))
        else:
            shapes = ((n, 16, "[>= n, 16]"), (m, 12, "[>= m, 12]"), (n + 1, None, "[>= n + 1]"))
            if len(out) != 3:
                raise ValueError("out must be (headers, records, offs)")
            for t, (rows, width, what) in zip(out, shapes):
                if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int32 or t.device != dev \
                        or not t.is_contiguous() or t.dim() != (1 if width is None else 2) or t.shape[0] < rows \
                        or (width is not None and t.shape[1] != width):
                    raise ValueError(f"out must be contiguous int32 tensors {what} on the headers' device")
        if status is None:
            status = torch.zeros(1, dtype=torch.int32, device=dev)
        elif not isinstance(status, torch.Tensor) or status.dtype != torch.int32 or status.numel() != 1 \
                or status.device != dev:
            raise ValueError("status must be an int32 [1] tensor on the headers' device")
        if work is None:
            work = torch.empty(max(16, need), dtype=torch.uint8, device=dev)
        elif not isinstance(work, torch.Tensor) or work.dtype != torch.uint8 or work.device != dev \
                or not work.is_contiguous() or work.numel() < need:
            raise ValueError(f"work must be a contiguous uint8 tensor of at least {need} bytes on the headers' device")
        check(lib().bgx_harvest_canonical(ptr(headers), ptr(records), n, m, lane_base, lanes, ptr(out[0]), ptr(out[1]),
                                          ptr(out[2]), ptr(status), ptr(work), work.numel(), stream_handle(s)),
              "bgx_harvest_canonical")
    return out[0][:n], out[1][:m], out[2][:n + 1]


def load_pth(path):
    """A reference checkpoint (torch.save of BackgammonPolicyNetwork.state_dict(),
    parameter_manager.py:115-151: fc1.weight / fc1.bias / value_head.weight /
    value_head.bias) -> dict of host fp32 W1, b1, w2, b2. Loaded with
    weights_only=True (no code from the file runs)."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    return dict(zip(("W1", "b1", "w2", "b2"), weights_from(sd)))
