#!/usr/bin/env python3
"""Turns the raw outputs of tools/refresh_profiles.sh (gpurun_out/prof_*) into the files committed under profiles/:
r06_bench.json (the full result; the stdout line is its short form), r06_rocprof_kernel_stats.txt, r06_pmc_summary.txt, pmc.json
(keyed to the kernel source hash), r06_getrow_config3.txt, r06_floor.txt."""
import hashlib, json, os, re, shutil, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RND = "r06"


def kernel_source_sha16():
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "libsmatrix_amd", "csrc")
    for f in ["smx_kernels.hpp"] + sorted(os.path.join("kernels", k) for k in os.listdir(os.path.join(csrc, "kernels")) if k.endswith(".hpp")) + ["smx_runtime.hip"]:
        h.update(open(os.path.join(csrc, f), "rb").read())
    return h.hexdigest()[:16]


G = os.path.join(ROOT, "gpurun_out"); P = os.path.join(ROOT, "profiles")
raw = open(os.path.join(G, "prof_pmc_raw.txt")).read()
AGG, GET = "smx::k_apply_agg<2, 1u, true, false>", "smx::k_apply<0, false>"   # (the instantiations of a matrix without a hint table)


def val(kern, grid, ctr):
    m = re.search(r"%s\s+grid=%s\s+%s\s+dispatches=\s*(\d+) mean=\s*([\d.]+)" % (re.escape(kern), grid, ctr), raw)
    return float(m.group(2))


agg = {k: val(AGG, "8388608", c) for k, c in (("fetch", "FETCH_SIZE"), ("write", "WRITE_SIZE"), ("hit", "TCC_HIT_sum"),
                                                ("miss", "TCC_MISS_sum"), ("atom", "TCC_EA0_ATOMIC_sum"))}
get = {k: val(GET, "16777216", c) for k, c in (("fetch", "FETCH_SIZE"), ("write", "WRITE_SIZE"), ("hit", "TCC_HIT_sum"),
                                                 ("miss", "TCC_MISS_sum"))}
p0 = val("smx::k_probe_random<0>", "2097152", "FETCH_SIZE")
b = json.load(open(os.path.join(G, "prof_bench.json")))
ra = b["random_access"]; R, A = ra["read8_gtouch_per_s"], ra["atomic_ret_gtouch_per_s"]
N = 1 << 24
bytes_agg = (agg["fetch"] + agg["write"]) * 1024; bytes_get = (get["fetch"] + get["write"]) * 1024
rd_agg = agg["miss"] - agg["atom"]
t_agg = rd_agg / (R * 1e9) + agg["atom"] / (A * 1e9); t_get = get["miss"] / (R * 1e9)
ki, kg = b["roofline"]["avg_launch_ms"], b["roofline_get"]["avg_launch_ms"]
hdr = """# rocprofv3 --kernel-trace --pmc <counter> --output-format csv -- python3 bench.py --full --no-cpu --no-extras   (three separate passes: FETCH_SIZE | WRITE_SIZE | TCC_HIT_sum TCC_MISS_sum TCC_EA0_ATOMIC_sum; tools/refresh_profiles.sh + tools/build_profiles.py)
# MI355X, round 6, bench.py --full --no-cpu --no-extras: config 2 = 24 batches of 2^24 ops (+ 4 replayed batches of the steady-state extra).  FETCH_SIZE/WRITE_SIZE are KiB per dispatch, means over the dispatches listed.
# Calibration in our own access pattern, same runs: k_probe_random<0> = 2^27 random 8-byte loads over 4 GiB -> %.0f KiB = %.1f B per touch
#   (a 64 B line per touch; no 1/2 correction for this shape); k_probe_random<1>/<2> = 2^27 scattered 32-bit atomics -> WRITE_SIZE 32 B and TCC_EA0_ATOMIC 1.0 per atomic.
#   (the guide's gfx950 correction -- FETCH_SIZE tallies a 128-B coalesced streaming request at 64 B -- applies only to the streamed op arrays,
#    12 B/op in for incr and 8 B/op for get: at most +6 / +4 B/op on the figures below; the random 8-16 B touches are counted in full, as calibrated)
# HBM-side traffic per launch of the op kernels (full-batch dispatches, 2^24 ops each):
#   k_apply_agg<INCR>: fetch %.1f KiB + write %.1f KiB = %.3e B = %.0f B/op (algorithmic 32 B/op); %.1f M memory-side atomics; L2 hit %.0f %%
#   k_apply<GET>     : fetch %.1f KiB + write %.1f KiB = %.3e B = %.0f B/op (algorithmic 24 B/op); L2 hit %.0f %%
#   (each op touches two 64-byte lines -- directory slot, cell -- of which ~half are served by L2; the 8-byte cell costs a 64-byte line)
# The memory-side bound of these transaction counts, priced with the random-touch rates measured in the bench run of the same box
# (read8 %.1f G/s, returning atomic %.1f G/s, uniform over 4 GiB).  TCC_MISS counts an atomic as a miss (probe<1>: 1.0 per atomic),
# so the read misses of the incr kernel are TCC_MISS - TCC_EA0_ATOMIC; they include the streamed op arrays (12 B/op in = 3.1 M lines).
#   k_apply_agg<INCR>: %.1f M read misses / %.1f G/s + %.1f M atomics / %.1f G/s = %.3f ms;  measured %.3f ms per launch (HIP events, growing table;
#                      1.30 ms when every key is a hit) -> %.0f %% of that bound.  The atomics are 80 %% of it: one returning atomic per distinct key of a
#                      2048-op tile (+ a ticket and a claim per new cell: the round-4 census counted 15.0 M + 3.8 M + 3.8 M for batch 15) -- the LDS fold removes the duplicates inside a tile, not across tiles
#                      (how the kernel's time splits over these classes: profiles/r02_agg_kernel_phase_shares.txt).
#   k_apply<GET>     : %.1f M misses / %.1f G/s = %.3f ms;  measured %.3f ms -> %.0f %%
#   i.e. the kernels run within 15-30 %% of the chip's random-transaction rates for what they touch; the rest of the gap to the byte roofline is the COUNT
#   (two lines per op, 64 B moved per 8-16 B used).
""" % (p0, p0 * 1024 / (1 << 27), agg["fetch"], agg["write"], bytes_agg, bytes_agg / N, agg["atom"] / 1e6,
       100 * agg["hit"] / (agg["hit"] + agg["miss"]), get["fetch"], get["write"], bytes_get, bytes_get / N,
       100 * get["hit"] / (get["hit"] + get["miss"]), R, A, rd_agg / 1e6, R, agg["atom"] / 1e6, A, t_agg * 1e3, ki,
       100 * t_agg * 1e3 / ki, get["miss"] / 1e6, R, t_get * 1e3, kg, 100 * t_get * 1e3 / kg)
open(os.path.join(P, RND + "_pmc_summary.txt"), "w").write(hdr + raw)
json.dump({"summary": "profiles/%s_pmc_summary.txt" % RND, "kernel_source_sha16": kernel_source_sha16(),
           "source": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE / TCC_* in separate passes of `python3 bench.py --full --no-cpu --no-extras`",
           "k_apply_agg_incr": {"fetch_kib": agg["fetch"], "write_kib": agg["write"], "bytes_per_launch": int(bytes_agg), "ops_per_launch": N,
                                "l2_misses": agg["miss"], "memory_side_atomics": agg["atom"]},
           "k_apply_get": {"fetch_kib": get["fetch"], "write_kib": get["write"], "bytes_per_launch": int(bytes_get), "ops_per_launch": N,
                           "l2_misses": get["miss"]}}, open(os.path.join(P, "pmc.json"), "w"), indent=1)
ur = json.load(open(os.path.join(G, "prof_bench_under_rocprof.json")))
open(os.path.join(P, RND + "_rocprof_kernel_stats.txt"), "w").write(
    "# rocprofv3 --kernel-trace --stats --output-format csv -- python3 bench.py --full --no-cpu --no-extras   (MI355X, round 6, tools/refresh_profiles.sh; bench line of this "
    "same profiled run: %.0f Mops/s, k_apply_agg<INCR> round-0 avg %.3f ms and k_apply<GET> %.3f ms by HIP events; the full-batch grids below include the 4 all-hit "
    "replays of the steady-state extra and the first batches of the empty table)\n" % (ur["value"], ur["roofline"]["avg_launch_ms"], ur["roofline_get"]["avg_launch_ms"])
    + open(os.path.join(G, "prof_kernel_stats.txt")).read()
    + "\n# per-step spans of the same trace (tools/step_spans.py): span, busy, idle, kernels, prep rounds | top kernels (us)\n"
    + open(os.path.join(G, "prof_step_spans.txt")).read() + "\n# kernel timeline of the last step of the growing table (tools/timeline.py <dir> last-growing)\n"
    + open(os.path.join(G, "prof_timeline_step23.txt")).read())
# the bench line must carry the traffic of THIS refresh: bench.py reads profiles/pmc.json, which was just rewritten
b["roofline"]["traffic"] = int(bytes_agg); b["roofline_get"]["traffic"] = int(bytes_get)
b["roofline"]["memory_side_atomics"] = agg["atom"]
for r in ("roofline", "roofline_get"):
    b[r].pop("traffic_note", None)      # that note was about the pmc.json this refresh has just replaced
    b[r]["traffic_source"] = "profiles/%s_pmc_summary.txt (PMC passes of this same refresh)" % RND
json.dump(b, open(os.path.join(P, RND + "_bench.json"), "w"))
print(hdr)
# config 3: the getrow scan
raw3 = open(os.path.join(G, "prof_pmc_raw_config3.txt")).read()
ks3 = open(os.path.join(G, "prof_kernel_stats_config3.txt")).read()
c3 = json.load(open(os.path.join(G, "prof_bench_config3_under_rocprof.json")))


def val3(kern, ctr):
    m = re.search(r"%s(?:<[^>]*>)?\s+grid=\d+\s+%s\s+dispatches=\s*(\d+) mean=\s*([\d.]+)" % (re.escape(kern), ctr), raw3)
    return float(m.group(2)) if m else None


f3, w3 = val3("smx::k_getrow", "FETCH_SIZE"), val3("smx::k_getrow", "WRITE_SIZE")
d3 = c3["result"]
lines = ["# config 3 (bench.py --config 3): smatrix_rowlen + smatrix_getrow over all %d rows / %d nnz of the CF matrix, MI355X, round 6" % (d3["rows"], d3["nnz"]),
         "# bench line of the profiled run: getrow %.3f ms = %.1f G nnz/s; algorithmic %.0f GB/s = %.3f of the 8 TB/s peak; build %.2f s (%.2f G ops/s)"
         % (d3["getrow_ms"], d3["Gnnz_per_s"], d3["roofline"]["achieved"], d3["roofline"]["frac"], d3["build_s"], d3["build_Gops_per_s"])]
if f3 and w3:
    # k_getrow streams the row tables with 16-byte loads: the guide's gfx950 correction applies (FETCH_SIZE tallies 128-B requests at 64 B)
    moved = f3 * 1024 * 2 + w3 * 1024
    lines.append("# PMC (separate passes): FETCH_SIZE %.0f KiB (x2 by the gfx950 streaming correction) + WRITE_SIZE %.0f KiB = %.3e B per launch"
                 " = %.2f TB/s over %.3f ms; model: %d B" % (f3, w3, moved, moved / (d3["getrow_ms"] * 1e-3) / 1e12, d3["getrow_ms"], d3["roofline"]["bytes_moved_model"]))
if f3 and w3:
    pj = json.load(open(os.path.join(P, "pmc.json")))
    pj["k_getrow"] = {"fetch_kib": f3, "write_kib": w3, "bytes_per_launch": int(moved), "rows": d3["rows"], "nnz": d3["nnz"],
                      "note": "FETCH_SIZE doubled (gfx950: 128-B streaming requests are tallied at 64 B)"}
    json.dump(pj, open(os.path.join(P, "pmc.json"), "w"), indent=1)
open(os.path.join(P, RND + "_getrow_config3.txt"), "w").write("\n".join(lines) + "\n" + ks3 + "\n" + raw3)
json.dump(c3, open(os.path.join(P, RND + "_bench_config3.json"), "w"))

# ---- the floor of the mixed step: fresh PMC counts x the probe rates of the same box, not prose
spans = open(os.path.join(G, "prof_step_spans.txt")).read()
tl = open(os.path.join(G, "prof_timeline_step23.txt")).read()
growth_us = 0.0
names = []
for ln in tl.splitlines():
    m = re.match(r"\s*([\d.]+) us\s+\+\s*([\d.]+)\s+(\S+)", ln)
    if m and not m.group(3).startswith("smx::k_apply_agg") and m.group(3) != GET and "copyBuffer" not in m.group(3):
        names.append((m.group(3), float(m.group(2))))
# critical path of the growth round: prep, plan, the longer of {three in-LDS rehash kinds in sequence} and {map, move, finish, zero on the
# helper stream}, commit, advance, retry, prep
def dur(prefix):
    return sum(v for k, v in names if k.startswith(prefix))
lds = dur("smx::k_grow_lds")
chunked = dur("smx::k_grow_map") + dur("smx::k_grow_move") + dur("smx::k_grow_finish") + dur("smx::k_grow_zero")
crit = dur("smx::k_prep") + dur("smx::k_grow_plan") + max(lds, chunked) + dur("smx::k_grow_commit") + dur("smx::k_round_advance") + dur("smx::k_apply<2")
steady = b.get("steady_state_all_hits", {})
ins = agg["atom"] - 15.0e6                                           # tickets + claims beyond one atomic per (tile, key) entry (census: 15.0 M entries)
floor_agg = t_agg * 1e3
floor_get = t_get * 1e3
lines_f = [
 "# The floor of one mixed step (incr batch + get batch of 2^24 ops each, config 2) of THIS design on THIS box -- round 6 (the kernels of the headline path are those of round 4: frozen).",
 "# Every count is a PMC mean of the committed passes (profiles/%s_pmc_summary.txt), every rate a probe of the same bench run" % RND,
 "# (random_access in profiles/%s_bench.json); nothing here is estimated from prose." % RND,
 "",
 "chip rates (uniform random over 4 GiB): read8 %.1f G/s, returning atomic %.1f G/s" % (R, A),
 "",
 "k_apply_agg<INCR>, one launch = 2^24 ops:",
 "  memory-side atomics (TCC_EA0_ATOMIC)        %6.2f M   / %.1f G/s = %.3f ms" % (agg["atom"] / 1e6, A, agg["atom"] / (A * 1e9) * 1e3),
 "  read misses (TCC_MISS - atomics)            %6.2f M   / %.1f G/s = %.3f ms" % (rd_agg / 1e6, R, rd_agg / (R * 1e9) * 1e3),
 "  transaction floor                                                     %.3f ms   (measured %.3f ms by HIP events: %.0f %% of the floor's rate)" % (floor_agg, ki, 100 * floor_agg / ki),
 "k_apply<GET>, one launch = 2^24 ops:",
 "  read misses (TCC_MISS)                      %6.2f M   / %.1f G/s = %.3f ms   (measured %.3f ms)" % (get["miss"] / 1e6, R, floor_get, kg),
 "growth round of a steady batch (kernel timeline of the last growing step of the same trace, critical path):",
 "  prep %.0f + plan %.0f + max(in-LDS rehash x3 %.0f, chunked passes %.0f) + commit %.0f + advance %.0f + retry %.0f us = %.3f ms"
 % (dur("smx::k_prep"), dur("smx::k_grow_plan"), lds, chunked, dur("smx::k_grow_commit"), dur("smx::k_round_advance"), dur("smx::k_apply<2"), crit / 1e3),
 "",
 "floor of the step with every kernel AT its transaction floor and no idle time:  %.3f + %.3f + %.3f = %.3f ms" % (floor_agg, floor_get, crit / 1e3, floor_agg + floor_get + crit / 1e3),
 "measured: %.3f ms per step over the timed steps (%.2f G mixed ops/s); all-hit replay %.3f ms" % (b["ms_per_step"], b["value"] / 1e3, steady.get("ms_per_step", float("nan"))),
 "target of north_star: 0.40 of read8 = %.3f ms per step" % (2 * N / (0.4 * R * 1e9) * 1e3),
 "",
 "What the counts are made of (round 4 census of batch 15 of the stream on the CPU; the probes are in the git history):",
 "  14.99 M (tile, key) entries for 7.01 M distinct keys: one verify load + one returning atomic each; 3.74 M of them are inserts",
 "  (+ one `used` ticket each, + the claim CAS instead of the add).  95.6 % of the entries have ONE op in their tile (85 % of the ops):",
 "  the LDS fold removes the hot cells' serialisation, not transactions.  6.07 M of the 7.01 M keys appear in one tile only; the 0.94 M",
 "  keys that appear in several tiles make up 8.92 M entries -- what a cross-tile fold would save, priced in rounds 2/3 at >= its own cost",
 "  on one GPU (a 1024-way key split + the un-permuting of results).",
 "  Ticket-free inserts (VERDICT r3 2b): 90.0 % of the inserts land in rows whose room covers the row's TRUE number of new keys, 73.5 % in rows",
 "  whose room covers the row's OP COUNT in the batch -- the only bound a kernel could hold, and computing it (a per-batch row histogram)",
 "  costs one atomic per (tile, row) pair, 7.98 M per batch (same census) against the 3.7 M tickets it would save.  Estimates from the previous batch cover",
 "  39-70 % but are not bounds: one row that overshoots its threshold breaks the reference's growth rule (src/smatrix.c:343-360).  Dropped.",
 "  Hot/cold split (2c): the whole LDS fold costs 0.14 ms of the kernel (profiles/r02_agg_kernel_phase_shares.txt) and the kernel already runs",
 "  8 waves per SIMD (two 1024-lane workgroups per CU): there is no third workgroup to win, whatever the table costs.  Dropped.",
 "  Round >= 1 in one launch (2a): the growth round's critical path above is kernel time, ~%.2f ms; grouping the ~230 000 deferred ops by row" % (crit / 1e3),
 "  (count, scan, scatter, rows) is five launches of its own -- round 2 measured that fixed cost at what the round costs today.  The bulk",
 "  path was widened where it pays instead: hot rows now give it their first 2048 ops (first incr batch of config 2: 13.0 -> 8.0 ms).",
]
open(os.path.join(P, RND + "_floor.txt"), "w").write("\n".join(lines_f) + "\n")
print("\n".join(lines_f))
