"""The adaptive half of a step with ONE RANK PER HOST THREAD, each calling for itself over the thread transport, in the two modes a rank
of a multi-process run has for it: the per-rank "compact" mode (include/sph_slab_partner_problem.h: every rank prepares and downloads its
local problem, the problems are merged in numpy, the host loop decides, the K decisions go back up to every rank) and the device mode
(include/sph_rank_partner_search.h: the local problems relayed to the root over the ranks' transport, merged and solved on its device,
the decisions relayed back).

configs[0] and configs[4] as scripts/gpu_slab_partner_problem_time.py builds them, on TWO RANKS of one device, a few adaptive steps per
mode from the same start, ONE PROCESS PER MODE AND RUN (fresh children of this script, one after the other, in one invocation).  Per pass
(one partner search and its apply) the wall time of its parts, taken on the host around the calls of all ranks together: compact --
`prepare`, `download`, `merge` (numpy), `decide` (the host loop), `apply`; device -- `find` (the one collective call: prepare, blob,
relay, merge, solve, relay) and `apply`.  With K, the solver's rounds, the relay's rounds and sub-rounds and the bytes the ranks passed
between their buffers.  The compact mode here hands the problems over inside one process: a launch with one process per rank also
pickles them through the launcher (torch.distributed gather_object / broadcast_object_list), which this baseline does NOT pay.
The event counts must be equal between the modes and the runs.  Every time is the median over the runs (smallest .. largest).
Writes <out-dir>/<name>.json and <name>.md.

    python scripts/gpu_rank_device_search_time.py [--configs 0 4] [--runs 3] [--steps 2] [--warmup 2] [--root 0] [--out-dir profiles]
                                                  [--name r14_rank_device_search_tables]
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "scripts"))
MODES = ("compact", "device")
PARTS = ("prepare_s", "download_s", "merge_s", "decide_s", "find_s", "apply_s")
RANKS = 2


def child(mode: str, config: int, steps: int, warmup: int, root: int) -> dict:
    import torch  # noqa: F401  (runtime load order, see ffi.load_product)
    from gpu_slab_partner_problem_time import setup
    from adaptive_sph_amd import adaptivity as A, distributed as D, ffi
    plib = ffi.load_product()
    desc, P, (pos, mass, vel, planes) = setup(config)
    tg = D.ThreadedGroup(plib, pos, mass, vel, planes, RANKS)
    grp = tg.contexts
    pool = ThreadPoolExecutor(RANKS)
    sp = A.SplitPatterns.load_from_file(REPO / "tests" / "golden" / "split-patterns.yaml")
    for c in grp:
        c.set_split_patterns(sp.patterns)
    p = P.to_ffi()

    def every(fn):
        return [f.result() for f in [pool.submit(fn, c) for c in grp]]

    def clocked(spent, part, fn):
        t0 = time.perf_counter()
        out = fn()
        spent[part] += time.perf_counter() - t0
        return out

    def search(kind, ap, dt):
        spent = dict.fromkeys(PARTS, 0.0)
        q = {"kind": kind}
        every(lambda c: c.classify(p))
        if mode == "device":
            found = clocked(spent, "find_s", lambda: every(lambda c: c.slab_find_partners_device(kind, p, ap, root=root)))
            sizes = [c.slab_relay_sizes() for c in grp]
            plan = ffi.relay_plan(plib, RANKS, root, 0, sizes[0]["bytes_of_rank"], sizes[0]["chunk_bytes"]) if found[0]["participants"] else []
            q.update(K=found[0]["participants"], candidates=found[0]["candidates"], rounds=found[0]["rounds"], transfers=found[0]["transfers"],
                     relay_rounds=len({s["round"] for s in plan}), relay_sub_rounds=len(plan), blobs=sizes[0]["bytes_of_rank"],
                     decisions_bytes=sizes[0]["decisions_bytes"], bytes_between_devices=sum(s["bytes_sent"] for s in sizes))
            clocked(spent, "apply_s", lambda: every(lambda c: c.slab_adapt_device(kind, p, ap)))
        else:
            clocked(spent, "prepare_s", lambda: every(lambda c: c.slab_partner_problem_prepare(kind, p, ap)))
            parts = clocked(spent, "download_s", lambda: every(lambda c: c.slab_partner_problem_download()))
            pids, *fields, off_c, idx_c = clocked(spent, "merge_s", lambda: D.merge_slab_partner_problems(parts))
            mp_c, mc_c = clocked(spent, "decide_s", lambda: D._decide_compact(plib, kind, pids, fields, off_c, idx_c, P, dt))
            q.update(K=len(pids), candidates=len(idx_c), rounds=0, transfers=int(mc_c.sum()), relay_rounds=0, relay_sub_rounds=0, blobs=[], decisions_bytes=0,
                     bytes_between_devices=0)
            apply = (lambda c: c.slab_share_particles_compact(p, ap, pids, mp_c, mc_c)) if kind == "share" else (lambda c: c.slab_merge_particles_compact(p, ap, pids, mp_c, mc_c))
            clocked(spent, "apply_s", lambda: every(apply))
        q.update(spent)
        return q

    for _ in range(warmup):
        tg.step(p)
    per_step = []
    for _ in range(steps):
        sts = tg.step(p)
        dt, num = float(sts[0].dt), int(sts[0].step_number)
        ap = A.adapt_params(P, dt)
        n = sum(c.n for c in grp)
        passes = []
        t0 = time.perf_counter()
        if P.sharing:
            passes.append(search("share", ap, dt))
        if num % 2 == 0:
            if P.merging:
                passes.append(search("merge", ap, dt))
        elif P.splitting:
            every(lambda c: c.classify(p))
            every(lambda c: c.split_particles(p, ap))
        wall = time.perf_counter() - t0
        per_step.append({"step_number": num, "n_before": n, "n_after": sum(c.n for c in grp), "adaptive_half_s": wall, "passes": passes,
                         "events": {"shares": sum(q["transfers"] for q in passes if q["kind"] == "share"),
                                    "merges": sum(q["transfers"] for q in passes if q["kind"] == "merge"), "splits": sum(c.n for c in grp) - n if num % 2 else 0}})
    out = {"mode": mode, "workload": desc, "ranks": RANKS, "root": root, "transport": grp[0].dist_get_stats()["transport"], "device": torch.cuda.get_device_name(0),
           "devices_used": 1, "per_step": per_step}
    pool.shutdown(wait=True)
    tg.close()
    return out


def spread(values) -> str:
    return f"{statistics.median(values):.4f} ({min(values):.4f} .. {max(values):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--root", type=int, default=0)
    ap.add_argument("--configs", type=int, nargs="+", default=[0, 4], choices=(0, 4))
    ap.add_argument("--out-dir", default=str(REPO / "profiles"))
    ap.add_argument("--name", default="r14_rank_device_search_tables")
    ap.add_argument("--child", choices=MODES)
    ap.add_argument("--config", type=int, default=4)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a.child, a.config, a.steps, a.warmup, a.root)))
        return
    res = {}
    for config in a.configs:
        for mode in MODES:
            for run in range(a.runs):
                r = subprocess.run([sys.executable, __file__, "--child", mode, "--config", str(config), "--steps", str(a.steps), "--warmup", str(a.warmup),
                                    "--root", str(a.root)], capture_output=True, text=True, timeout=600)
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
                if r.returncode != 0 or not line:
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    raise SystemExit(f"configs[{config}] mode {mode} run {run} failed (exit {r.returncode})")
                res.setdefault(str(config), {}).setdefault(mode, []).append(json.loads(line[-1][7:]))
                print(f"configs[{config}] {mode} run {run}: done", flush=True)
    out = Path(a.out_dir)
    out.mkdir(parents=True, exist_ok=True)
    (out / (a.name + ".json")).write_text(json.dumps(res, indent=1) + "\n")
    md = []
    for config in a.configs:
        R = res[str(config)]
        ev = [[s["events"] for s in run["per_step"]] for m in MODES for run in R[m]]
        assert all(e == ev[0] for e in ev), ("the modes or the runs took different decisions", ev)
        first = R["compact"][0]
        md += [f"## {first['workload']}", "",
               f"{RANKS} ranks on host threads over the {first['transport']} transport, all on ONE {first['device']}; root {a.root}; one process per mode and run in one "
               f"invocation, {a.warmup} plain steps, then {a.steps} adaptive steps; {a.runs} runs per mode.  `compact` is the baseline.  Seconds of wall time on the host, "
               "around the calls of all ranks together: the median of the runs (smallest .. largest).", "",
               "| step | pass | mode | K | candidates | solver rounds | relay rounds / sub-rounds | blobs (bytes per rank) | bytes between devices | prepare | download | merge | decide | find (one call) | apply | pass total |",
               "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for k in range(len(first["per_step"])):
            for m in MODES:
                runs = [run["per_step"][k]["passes"] for run in R[m]]
                for j, q in enumerate(runs[0]):
                    cols = " | ".join(spread([r[j][part] for r in runs]) if any(r[j][part] for r in runs) else "-" for part in PARTS)
                    total = spread([sum(r[j][part] for part in PARTS) for r in runs])
                    md.append(f"| {R[m][0]['per_step'][k]['step_number']} | {q['kind']} | {m} | {q['K']} | {q['candidates']} | {q['rounds'] or '-'} | "
                              f"{q['relay_rounds']} / {q['relay_sub_rounds']} | {q['blobs'] or '-'} | {q['bytes_between_devices'] or '-'} | {cols} | {total} |")
        md += ["", "| step | events (shares / merges / splits) | mode | adaptive half |", "|---|---|---|---|"]
        for k in range(len(first["per_step"])):
            for m in MODES:
                runs = [run["per_step"][k] for run in R[m]]
                e = runs[0]["events"]
                md.append(f"| {runs[0]['step_number']} | {e['shares']} / {e['merges']} / {e['splits']} | {m} | {spread([q['adaptive_half_s'] for q in runs])} |")
        md.append("")
    (out / (a.name + ".md")).write_text("\n".join(md) + "\n")
    print("\n".join(md))


if __name__ == "__main__":
    main()
