#!/usr/bin/env python3
"""State across batches on the device, timed.

Cost of the carry, at §9c's cells (RECORDS PLACED records of 1460 B in random
flow order over FLOWS flows, 1 % of them twice):

  plain       lvlip_lro_advance_dev (device events)
  carry_null  lvlip_lro_advance_carry_dev with prev == NULL (device events)
  carry_live  lvlip_lro_advance_carry_dev with four live carried blocks per
              flow, beyond the records (device events)

One receive round at FRAMES records over 1024 flows:

  round_dev   lvlip_lro_advance_carry_dev -> lvlip_ack_dev -> lvlip_lro_next_dev
              on one stream (device events); the flows are put back by a
              device copy outside the events
  round_host  the host-step form: lvlip_lro_advance_dev -> lvlip_ack_dev, then
              the results to pinned host memory, a synchronise, the update on
              the host (numpy) and the flows back to the device (wall)

(lvlip_lro_dev itself is the same in both and is left out: scripts/lro_bench.py
has it.)  Forms alternate in one process after warm-up rounds (median, min,
max).  Before anything is timed, every device result is checked equal, byte for
byte, to the host form's.

    python scripts/carry_bench.py [--records N ...] [--flows N ...] [--warmup W] [--repeats R] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "level-ip_amd"))

import torch  # noqa: E402

import lvlip  # noqa: E402
from lro_advance_bench import _dev, spread, wall_ms  # noqa: E402
from tso_bench import timed  # noqa: E402

MSS = 1460
M32 = 0xFFFFFFFF


def cell(n: int, nflows: int):
    """(flows, rec, prev): prev's four blocks per flow lie behind the records."""
    rng = np.random.default_rng(n + nflows)
    k = np.arange(nflows)
    flows = np.zeros(nflows, dtype=lvlip.LRO_FLOW_DTYPE)
    flows["saddr"], flows["daddr"] = 0x0500000A, 0x0400000A
    flows["sport"], flows["dport"] = ((k & 0xFF) << 8) | (k >> 8), 0x401F
    flows["rcv_nxt"], flows["rcv_wnd"], flows["out_off"], flows["user"] = 0xFFFFFF00, 1 << 24, k.astype(np.uint64) << 24, k
    lvlip.lro_plan(flows)
    ids = rng.permutation(n - n // 100)
    ids = np.concatenate([ids, ids[:n // 100]])
    ids = ids[rng.permutation(n)]
    rec = np.zeros(n, dtype=lvlip.LRO_REC_DTYPE)
    rec["flow"], rec["rel"] = ids % nflows, (ids // nflows) * MSS
    rec["dlen"], rec["status"], rec["tcp_flags"] = MSS, lvlip.LRO_PLACED, 0x10
    top = (n // nflows + 2) * MSS
    prev = np.zeros(nflows, dtype=lvlip.LRO_RESULT_DTYPE)
    prev["nsack"] = 4
    for j in range(4):
        prev["sack"][:, j, 0] = (flows["rcv_nxt"].astype(np.uint64) + top + 200000 * j) & M32
        prev["sack"][:, j, 1] = (flows["rcv_nxt"].astype(np.uint64) + top + 200000 * j + 70000) & M32
    return flows, rec, prev


class Cell:
    def __init__(self, n, nflows, dev):
        self.dev = dev
        self.flows, self.rec, self.prev = cell(n, nflows)
        self.f_t, self.rec_t, self.prev_t = (_dev(a, dev) for a in (self.flows, self.rec, self.prev))
        self.res_t = torch.zeros(48 * nflows, dtype=torch.uint8, device=dev)
        self.ws_plain = torch.empty(lvlip.lro_advance_workspace_bytes(n, nflows), dtype=torch.uint8, device=dev)
        self.ws_carry = torch.empty(lvlip.lro_advance_carry_workspace_bytes(n, nflows), dtype=torch.uint8, device=dev)

    def plain(self):
        lvlip.lro_advance_dev(self.f_t, self.rec_t, self.res_t, self.ws_plain)

    def carry_null(self):
        lvlip.lro_advance_carry_dev(self.f_t, self.rec_t, None, self.res_t, self.ws_carry)

    def carry_live(self):
        lvlip.lro_advance_carry_dev(self.f_t, self.rec_t, self.prev_t, self.res_t, self.ws_carry)

    def check(self):
        plain = lvlip.lro_advance(self.flows, self.rec)
        for form, want in (("plain", plain), ("carry_null", plain),
                           ("carry_live", lvlip.lro_advance_carry(self.flows, self.rec, self.prev))):
            self.res_t.fill_(0x5A)
            getattr(self, form)()
            torch.cuda.synchronize(self.dev)
            if self.res_t.cpu().numpy().tobytes() != want.tobytes():
                raise SystemExit(f"{form}: the device's results differ from the host form's")
        return int(want["nsack"].sum())


class Round(Cell):
    """One receive round behind lvlip_lro_dev, both ways."""

    def __init__(self, n, nflows, dev):
        super().__init__(n, nflows, dev)
        tmpl = np.zeros(nflows, dtype=lvlip.ACK_TMPL_DTYPE)
        hdr = np.zeros(54, dtype=np.uint8)
        hdr[12:15], hdr[23], hdr[46] = (0x08, 0x00, 0x45), 6, 0x50
        tmpl["hdr"], tmpl["max_sack"], tmpl["out_off"] = hdr, 4, np.arange(nflows, dtype=np.uint64) * 96
        tmpl["hdr"][:, 26:30] = self.flows["daddr"].copy().view(np.uint8).reshape(-1, 4)
        tmpl["hdr"][:, 30:34] = self.flows["saddr"].copy().view(np.uint8).reshape(-1, 4)
        tmpl["hdr"][:, 34:36] = self.flows["dport"].copy().view(np.uint8).reshape(-1, 2)
        tmpl["hdr"][:, 36:38] = self.flows["sport"].copy().view(np.uint8).reshape(-1, 2)
        self.ack_bytes = lvlip.ack_plan(tmpl, self.flows)
        self.tmpl_t = _dev(tmpl, dev)
        self.ack_t = torch.zeros(self.ack_bytes + 64, dtype=torch.uint8, device=dev)
        self.f0_t = self.f_t.clone()
        self.pinned = torch.empty(48 * nflows, dtype=torch.uint8).pin_memory()
        self.res_h = self.pinned.numpy().view(lvlip.LRO_RESULT_DTYPE)
        self.work = self.flows.copy()

    def reset(self):
        self.f_t.copy_(self.f0_t)
        self.res_t.copy_(self.prev_t)

    def round_dev(self):
        lvlip.lro_advance_carry_dev(self.f_t, self.rec_t, self.res_t, self.res_t, self.ws_carry)
        lvlip.ack_dev(self.tmpl_t, self.f_t, self.res_t, lvlip.ACK_ALL, self.ack_t)
        lvlip.lro_next_dev(self.f_t, self.res_t)

    def round_host(self):
        lvlip.lro_advance_dev(self.f_t, self.rec_t, self.res_t, self.ws_plain)
        lvlip.ack_dev(self.tmpl_t, self.f_t, self.res_t, lvlip.ACK_ALL, self.ack_t)
        self.pinned.copy_(self.res_t, non_blocking=True)
        torch.cuda.synchronize(self.dev)
        d = np.minimum(self.res_h["delivered"], self.work["rcv_wnd"])
        self.work["rcv_nxt"] += d
        self.work["out_off"] += d
        self.work["rcv_wnd"] -= d
        self.f_t.copy_(torch.from_numpy(self.work.view(np.uint8).reshape(-1)), non_blocking=True)
        torch.cuda.synchronize(self.dev)
        self.work[:] = self.flows

    def check_round(self):
        self.reset()
        self.round_dev()
        torch.cuda.synchronize(self.dev)
        f, r = self.flows.copy(), self.prev.copy()
        lvlip.lro_advance_carry(f, self.rec, r, r)
        lvlip.lro_next_cpu(f, r)
        if self.f_t.cpu().numpy().tobytes() != f.tobytes() or self.res_t.cpu().numpy().tobytes() != r.tobytes():
            raise SystemExit("round_dev: flows or results differ from the host forms'")


def time_forms(obj, forms, warmup, repeats, dev, before=None):
    stream = torch.cuda.current_stream(dev)
    t = {k: [] for k in forms}
    for r in range(warmup + repeats):
        for k, wall in forms.items():  # alternating, one process
            if before:
                before()
            torch.cuda.synchronize(dev)
            ms = wall_ms(getattr(obj, k)) if wall else timed(getattr(obj, k), stream)
            if r >= warmup:
                t[k].append(ms)
    return {k: spread(v) for k, v in t.items()}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, nargs="*", default=[256, 4096, 1 << 20])
    ap.add_argument("--flows", type=int, nargs="*", default=[1024, 65536])
    ap.add_argument("--rounds", type=int, nargs="*", default=[4096, 1 << 20])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available() or lvlip.device_count() == 0:
        raise SystemExit("carry_bench needs a HIP device (nothing is timed on the CPU)")
    dev = torch.device("cuda", 0)
    cells = {}
    for n in args.records:
        for nflows in args.flows:
            c = Cell(n, nflows, dev)
            islands = c.check()
            t = time_forms(c, {"plain": False, "carry_null": False, "carry_live": False}, args.warmup, args.repeats, dev)
            cells[f"{n}x{nflows}"] = {"records": n, "flows": nflows, "elements_with_carry": n + 4 * nflows,
                                      "islands_reported": islands, "equal_to_host_forms": True, "ms": t,
                                      "workspace_bytes": {"plain": c.ws_plain.numel(), "carry": c.ws_carry.numel()}}
            del c
            torch.cuda.empty_cache()
    rounds = {}
    for n in args.rounds:
        r = Round(n, 1024, dev)
        r.check()
        r.check_round()
        t = time_forms(r, {"round_dev": False, "round_host": True}, args.warmup, args.repeats, dev, before=r.reset)
        rounds[str(n)] = {"records": n, "flows": 1024, "equal_to_host_forms": True, "ms": t,
                          "ratio_host_over_dev": round(t["round_host"]["median"] / t["round_dev"]["median"], 2)}
        del r
        torch.cuda.empty_cache()
    res = {"script": "scripts/carry_bench.py", "device": torch.cuda.get_device_name(dev), "build_id": lvlip.BUILD_ID,
           "warmup": args.warmup, "repeats": args.repeats,
           "forms": {"plain": "lvlip_lro_advance_dev (device events)",
                     "carry_null": "lvlip_lro_advance_carry_dev, prev NULL (device events)",
                     "carry_live": "lvlip_lro_advance_carry_dev, four live blocks per flow (device events)",
                     "round_dev": "advance_carry_dev -> ack_dev -> lro_next_dev (device events)",
                     "round_host": "advance_dev -> ack_dev, results D2H, synchronise, host update, flows H2D (wall)"},
           "cells": cells, "rounds": rounds}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
