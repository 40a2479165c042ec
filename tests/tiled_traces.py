"""What the row-tiled drivers ENQUEUE, as comparable sequences: the cases and the recorders that tools/record_tiled_traces.py
(which writes tests/golden/tiled_traces.npz) and tests/test_tiled_steps.py (which holds the library to it) share.

Two kinds of trace, both free of addresses:
  * the audit log of a pm_tiled plan on logical devices (include/pm/testing.h), one row per runtime call, without the
    SET_DEVICE records: hipSetDevice is an idempotent host call that the two schedules placed differently;
  * what python/tiled.py::match_band asks of its comm (shift / send / recv / any) and of its engine (tile_*), per rank,
    with the integer arguments and whether an optional pointer was given.
"""
import threading

import numpy as np

ROWS, COLS, PATCH, ITERS, SEED = 150, 200, 5, 2, 91   # the pair of tests/test_tiled_devices.py
AUDIT_FIELDS = ("call", "band", "detail", "current_device", "stream_device", "object_device", "source_device",
                "foreign_allowed", "violation")
SET_DEVICE = 1
SPECULATIVE, PIPELINED = 0, 1


def _audit_cases():
    cases = []
    # every band count, every schedule and round count (0 forces the repeat; the pipelined schedule ignores rounds)
    for n in (1, 2, 3, 4, 7):
        for schedule, rounds in ((SPECULATIVE, -1), (SPECULATIVE, 1), (SPECULATIVE, 0), (PIPELINED, -1)):
            cases.append(dict(logical=list(range(n)), schedule=schedule, rounds=rounds, exchange=0, peer=0))
    # every way a row can cross: exchange mode x peer access x bands sharing a device or not, in both schedules
    for logical in ([0, 1, 2, 3], [0, 0, 1, 1]):
        for exchange in (0, 1, 2):
            for peer in (0, 1):
                for schedule, rounds in ((SPECULATIVE, -1), (SPECULATIVE, 0), (PIPELINED, -1)):
                    c = dict(logical=logical, schedule=schedule, rounds=rounds, exchange=exchange, peer=peer)
                    if c not in cases:
                        cases.append(c)
    for c in cases:
        c.update(matches=1, inject=0)
    # a second match on the same plan: buffers, events and `unread` hand-overs are reused
    for schedule, rounds in ((SPECULATIVE, 1), (SPECULATIVE, 0), (PIPELINED, -1)):
        for exchange, peer in ((0, 0), (2, 1)):
            cases.append(dict(logical=[0, 1, 2, 3], schedule=schedule, rounds=rounds, exchange=exchange, peer=peer,
                              matches=2, inject=0))
    # pm_tiled_debug_inject(1): the extra event record sits where a reader marks a row as consumed
    for schedule in (SPECULATIVE, PIPELINED):
        cases.append(dict(logical=[0, 0, 1, 1], schedule=schedule, rounds=-1, exchange=0, peer=1, matches=1, inject=1))
    return cases


AUDIT_CASES = _audit_cases()
DRIVER_CASES = [dict(world=w, pipelined=p, rounds=r) for w in (2, 3, 4) for p in (False, True) for r in (0, 1, 2)]


def audit_id(c):
    return "bands{}_dev{}_s{}_r{}_x{}_p{}_m{}_i{}".format(
        len(c["logical"]), "".join(map(str, c["logical"])), c["schedule"], c["rounds"], c["exchange"], c["peer"],
        c["matches"], c["inject"]).replace("-", "m")


def driver_id(c):
    return "ranks{}_{}_r{}".format(c["world"], "pipelined" if c["pipelined"] else "speculative", c["rounds"])


def pair(synth):
    p = synth.make_pair(SEED, rows=ROWS, cols=COLS, n_points=60, dilate_factor=3)
    return p["left"], p["right"], p["seed_l"], p["seed_r"]


def params(pm):
    return pm.default_params(0, patch=PATCH, patchmatch_iters=ITERS)


def audit_trace(pm, images, c):
    """One plan, c["matches"] matches: ([log of every match as an int16 array of AUDIT_FIELDS columns], [info as
    (rounds, repeated, exchanges)], [violations], [(disp_l, disp_r)])."""
    logs, infos, bad, maps = [], [], [], []
    with pm.TiledEngine(params(pm), ROWS, COLS, len(c["logical"]), logical_devices=c["logical"],
                        simulate_peer_access=c["peer"], exchange=c["exchange"], schedule=c["schedule"]) as t:
        if c["inject"]:
            t.debug_inject(c["inject"])
        for _ in range(c["matches"]):
            t.audit_reset()
            dl, dr, info = t.match(*images, rounds=c["rounds"])
            recs, violations = t.audit()
            logs.append(np.array([[r[f] for f in AUDIT_FIELDS] for r in recs if r["call"] != SET_DEVICE], np.int16))
            infos.append((info["rounds"], int(info["repeated"]), info["exchanges"]))
            bad.append(violations)
            maps.append((dl, dr))
    return logs, infos, bad, maps


def pack(arrays):
    """{name: 2-D integer array} -> the four arrays of the fixture (one zip member per trace would be mostly zip headers)."""
    names = sorted(arrays)
    return {"names": np.array(names), "shapes": np.array([arrays[k].shape for k in names], np.int32),
            "values": np.concatenate([np.asarray(arrays[k], np.int16).ravel() for k in names])}


def unpack(npz):
    shapes = npz["shapes"]
    ends = np.cumsum(shapes[:, 0] * shapes[:, 1])
    return {str(k): npz["values"][e - r * c:e].reshape(r, c) for k, (r, c), e in zip(npz["names"], shapes, ends)}


# ---- the Python driver -----------------------------------------------------------------------------------------------
WIDTH = 8   # a call: its kind, then up to seven integers, padded with -1
KINDS = ("shift", "send", "recv", "any", "tile_begin", "tile_noise", "tile_sweep", "tile_presweep", "tile_exchange_round",
         "tile_row_moved", "tile_get_row", "tile_set_row", "tile_background", "tile_finish")


def driver_trace(pm, tiled, images, c):
    """match_tiled_local with recording proxies in place of LocalComm and the engine: ([calls of rank k as an int16 array of
    WIDTH columns], disp_l, disp_r, info)."""
    calls, rank_of = {}, {}

    def note(kind, *ints):
        row = [KINDS.index(kind)] + [int(i) for i in ints]
        calls.setdefault(threading.get_ident(), []).append(row + [-1] * (WIDTH - len(row)))

    class Comm(tiled.LocalComm):
        def __init__(self, shared, rank):
            super().__init__(shared, rank)
            rank_of[threading.get_ident()] = rank

        def shift(self, row, down, send=True, recv=True):
            note("shift", down, send, recv)
            return super().shift(row, down, send=send, recv=recv)

        def send(self, row, dst, down=True):
            note("send", dst, down)
            return super().send(row, dst, down)

        def recv(self, like_shape, device, src, down=True):
            note("recv", src, down)
            return super().recv(like_shape, device, src, down)

        def any(self, flag_tensor):
            note("any")
            return super().any(flag_tensor)

    given = lambda p: 0 if p is None else 1

    class Engine(pm.Engine):
        def tile_begin(self, tile, d_left, d_right, band_rows, cols, d_seed_l, d_seed_r):
            note("tile_begin", tile.global_rows, tile.band_row0, tile.own_row0, tile.own_rows, band_rows, cols,
                 2 * given(d_seed_l) + given(d_seed_r))
            return super().tile_begin(tile, d_left, d_right, band_rows, cols, d_seed_l, d_seed_r)

        def tile_noise(self, it):
            note("tile_noise", it)
            return super().tile_noise(it)

        def tile_sweep(self, it, k):
            note("tile_sweep", it, k)
            return super().tile_sweep(it, k)

        def tile_presweep(self, pred_image_row, d_row):
            note("tile_presweep", pred_image_row, given(d_row))
            return super().tile_presweep(pred_image_row, d_row)

        def tile_exchange_round(self, it, k, pred_image_row, d_incoming, d_used, d_used_next, d_mask):
            note("tile_exchange_round", it, k, pred_image_row, d_incoming == d_used_next, d_incoming == d_used)
            return super().tile_exchange_round(it, k, pred_image_row, d_incoming, d_used, d_used_next, d_mask)

        def tile_row_moved(self, image_row, d_ref_row, d_flag):
            note("tile_row_moved", image_row)
            return super().tile_row_moved(image_row, d_ref_row, d_flag)

        def tile_get_row(self, image_row, d_dst):
            note("tile_get_row", image_row)
            return super().tile_get_row(image_row, d_dst)

        def tile_set_row(self, image_row, d_src):
            note("tile_set_row", image_row)
            return super().tile_set_row(image_row, d_src)

        def tile_background(self):
            note("tile_background")
            return super().tile_background()

        def tile_finish(self, d_out_l, d_out_r):
            note("tile_finish", given(d_out_r))
            return super().tile_finish(d_out_l, d_out_r)

    kept = tiled.LocalComm, pm.Engine
    tiled.LocalComm, pm.Engine = Comm, Engine
    try:
        dl, dr, info = tiled.match_tiled_local(params(pm), *images, c["world"], rounds=c["rounds"],
                                               pipelined=c["pipelined"])
    finally:
        tiled.LocalComm, pm.Engine = kept
    by_rank = {rank_of[t]: np.array(rows, np.int16) for t, rows in calls.items()}
    return [by_rank[k] for k in range(c["world"])], dl, dr, info
