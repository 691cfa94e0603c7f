#!/bin/bash
# All profiling passes of one round on the GPU box (gpurun -- 'bash tools/profile_round.sh r03'), per BASELINE configuration
#   ns    T=20 N=200 static   (north star)        n20   T=20 N=20        n2000  T=20 N=2000 (scaling point, one GPU)
#   c4    T=30 N=200 moving   (dynamic_obs)       ip    north star in the interior-point LamMuZ mode (row-parallel kernel, mu = 1e-3)
#   1. rocprofv3 --kernel-trace --stats                                   -> <cfg>_kernel_stats.csv, <cfg>_bench_under_rocprof.json
#   2. rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, one pass each (kernel-trace only) -> pmc_fetch_write.txt (all configs), <cfg>_bench_pmc_*.json
#   3. SQ issue counters, four passes (ns and c4)                           -> <cfg>_issue_counters.txt
#   4. plain bench runs (no profiler) of every config + the C5 fleet + the su phase profiles -> bench_<cfg>.json, suprof_<cfg>.txt
# then `python tools/profile_collect.py <tag>` (CPU) turns that into the committed summaries under profiles/.
TAG=${1:-r05}
cd /tmp && export TMPDIR=/tmp
cd "${GRAFT_REPO_ROOT:-/root/repo}" || exit 1
OUT="gpurun_out/prof_${TAG}"
mkdir -p "$OUT" "$OUT/scratch"
SCR="$OUT/scratch"
# Since round 5 every profiled process runs bench.py --only-headline: the headline closed loop (the reference's default protocol: re-sorted every tick)
# of the configuration and its hipEvent timing pass - the same kernels in the same protocol - and NOTHING else, so that the kernel averages of the
# rocprofv3 summary x launches per step reproduce ms_per_step of the line printed by the same process
BENCH="python bench.py --only-headline"
declare -A ARGS=( [ns]="--steps 100 --warmup 10" [n20]="--n-obs 20 --steps 100 --warmup 10" [n2000]="--n-obs 2000 --steps 60 --warmup 5" [c4]="--moving --horizon 30 --steps 60 --warmup 5" [ip]="--steps 60 --warmup 5" )
declare -A ENVS=( [ip]="RDA_LMZ_MODE=1 RDA_LMZ_MU=1e-3" )

: > "$OUT/pmc_fetch_write.txt"
for CFG in ns n20 n2000 c4 ip; do
  A="${ARGS[$CFG]}"; E="${ENVS[$CFG]}"
  D="$SCR/stats_$CFG"; mkdir -p "$D"
  env $E rocprofv3 --kernel-trace --stats --output-format csv -d "$D" -o bench -- $BENCH $A > "$D/run.log" 2>&1 || true
  grep '^{' "$D/run.log" | tail -1 > "$OUT/${CFG}_bench_under_rocprof.json" || true
  find "$D" -name '*kernel_stats.csv' -exec cp {} "$OUT/${CFG}_kernel_stats.csv" \;
  for C in FETCH_SIZE WRITE_SIZE; do
    D="$SCR/pmc_${CFG}_$C"; mkdir -p "$D"
    env $E rocprofv3 --kernel-trace --pmc $C --output-format csv -d "$D" -o pmc -- $BENCH $A --steps 40 > "$D/bench.log" 2>&1 || true
    grep '^{' "$D/bench.log" | tail -1 > "$OUT/${CFG}_bench_pmc_$C.json" || true
    find "$D" -name '*counter_collection.csv' -exec cp {} "$D/counters.csv" \;
    python - "$D/counters.csv" $C $CFG >> "$OUT/pmc_fetch_write.txt" <<'PY'
import csv, sys, collections
path, cname, cfg = sys.argv[1], sys.argv[2], sys.argv[3]
vals = collections.defaultdict(list)
try:
    for row in csv.DictReader(open(path)):
        if row.get("Counter_Name") == cname:
            vals[row["Kernel_Name"].split("(")[0]].append(float(row["Counter_Value"]))
    for k, v in vals.items():
        # launches queued behind the early-stop flag return at once and move (almost) nothing: an EXECUTED dispatch is one that moved
        # more than 0.4 of a LARGE dispatch of that kernel - the 98th percentile, not the maximum: the very first step of a handle is an
        # outlier (no remembered supports: every row goes through the enumeration, the work-list kernel moves 100 x its usual bytes)
        top = sorted(v)[max(0, int(0.98 * len(v)) - 1)]
        ex = [x for x in v if x > 0.4 * top and x <= 1.5 * top] or v
        # `steady`: everything except the first-step outliers (> 3 x the 90th percentile).  The work-list kernel of the split LamMuZ form
        # moves next to nothing in steady state (empty or short list) and 100 x that on a handle's first step, which then IS its 98th
        # percentile: its bytes per executed iteration are steady-total / executed launches of the common-path kernel (profile_collect.py)
        p90 = sorted(v)[max(0, int(0.90 * len(v)) - 1)]
        st = [x for x in v if x <= 3.0 * p90] or v
        print(f"{cfg} {cname} {k}: dispatches {len(v)} total {sum(v):.1f} per-dispatch {sum(v)/len(v):.3f} executed {len(ex)} per-executed {sum(ex)/len(ex):.3f} steady-total {sum(st):.1f}")
except Exception as e:
    print(cfg, "parse failed", e)
PY
  done
done

for CFG in ns c4; do
  A="${ARGS[$CFG]}"
  : > "$OUT/${CFG}_issue_counters.txt"
  G=0
  for GROUP in "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD" \
               "SQ_INSTS_VALU_FMA_F64 SQ_INSTS_VALU_MUL_F64 SQ_INSTS_VALU_ADD_F64 SQ_INSTS_VALU_TRANS_F64" \
               "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU" \
               "SQ_WAIT_INST_LDS SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_INSTS_SMEM"; do
    G=$((G + 1))
    D="$SCR/issue_${CFG}_$G"; mkdir -p "$D"
    rocprofv3 --kernel-trace --pmc $GROUP --output-format csv -d "$D" -o pmc -- $BENCH $A --steps 40 > "$D/bench.log" 2>&1 || true
    find "$D" -name '*counter_collection.csv' -exec cp {} "$D/counters.csv" \;
    python - "$D/counters.csv" >> "$OUT/${CFG}_issue_counters.txt" <<'PY'
import csv, sys, collections
vals = collections.defaultdict(list)
try:
    for row in csv.DictReader(open(sys.argv[1])):
        vals[(row["Kernel_Name"].split("(")[0], row["Counter_Name"])].append(float(row["Counter_Value"]))
    for k in sorted(vals):
        if "k_su" in k[0] or "k_lammuz" in k[0] or "k_lmz" in k[0]:
            v = vals[k]
            # an EXECUTED dispatch: more than 0.02 of a large one (98th percentile) of that kernel and counter - launches queued behind the early-stop
            # flag return at once and issue next to nothing (a cheap su-solve still issues a tenth of a hard one)
            top = sorted(v)[max(0, int(0.98 * len(v)) - 1)]
            ex = [x for x in v if x > 0.02 * top] or v
            print(f"{k[0]:28s} {k[1]:28s} dispatches {len(v):5d} per-dispatch {sum(v)/len(v):14.1f} executed {len(ex):5d} per-executed {sum(ex)/len(ex):14.1f}")
except Exception as e:
    print("parse failed", e)
PY
  done
done

timeout 400 python bench.py --full --egos 16 --fleet-egos 64 2> /dev/null | grep '^{' > "$OUT/bench_ns.json"                 # 200-step window, every leg, sizes
S0=$SECONDS
timeout 200 python bench.py --full --steps 20 --warmup 5 2> /dev/null | grep '^{' > "$OUT/bench_ns_driver_window.json"        # the driver's window, every leg
echo "wall clock of the driver's window with every leg (python bench.py --full --steps 20 --warmup 5): $((SECONDS - S0)) s" > "$OUT/driver_window_wall.txt"
for CFG in n20 n2000 c4; do timeout 300 python bench.py --full --no-sizes --egos 0 --fleet-egos 0 --no-ip-legs --cpu-threads 16 ${ARGS[$CFG]} 2> /dev/null | grep '^{' > "$OUT/bench_${CFG}.json"; done
timeout 300 python bench.py --full --no-cpu-baseline --no-sizes --no-ip-legs --egos 0 --fleet-egos 64 --n-obs 100 --horizon 25 2> /dev/null | grep '^{' > "$OUT/bench_c5_fleet.json"
D="$SCR/stats_c5"; mkdir -p "$D"
rocprofv3 --kernel-trace --stats --output-format csv -d "$D" -o f -- python bench.py --full --no-cpu-baseline --no-sizes --no-ip-legs --egos 0 --fleet-egos 64 --n-obs 100 --horizon 25 --steps 100 > /dev/null 2>&1 || true
find "$D" -name '*kernel_stats.csv' -exec cp {} "$OUT/c5_fleet_kernel_stats.csv" \;
# (the phase counters live in the profiling builds: tools/_bin/librda_hip_prof.so = -DSU_PROF, librda_hip_fine.so = -DSU_FINE, same sources)
RDA_HIP_SO=$PWD/tools/_bin/librda_hip_prof.so python tools/su_phase_profile.py > "$OUT/suprof_ns_fixed_binding.txt" 2>&1
RDA_HIP_SO=$PWD/tools/_bin/librda_hip_prof.so python tools/su_phase_profile.py --order > "$OUT/suprof_ns.txt" 2>&1
RDA_HIP_SO=$PWD/tools/_bin/librda_hip_prof.so python tools/su_phase_profile.py --n-obs 2000 --steps 60 --order > "$OUT/suprof_n2000.txt" 2>&1
RDA_HIP_SO=$PWD/tools/_bin/librda_hip_prof.so python tools/su_phase_profile.py --moving --horizon 30 --steps 60 --order > "$OUT/suprof_c4.txt" 2>&1
if [ -f tools/_bin/librda_hip_fine.so ]; then      # -DSU_FINE build of the same sources (sub-phases of the iteration)
  RDA_HIP_SO=$PWD/tools/_bin/librda_hip_fine.so python tools/su_phase_profile.py --order --fine > "$OUT/suprof_ns_fine.txt" 2>&1
  RDA_HIP_SO=$PWD/tools/_bin/librda_hip_fine.so python tools/su_phase_profile.py --moving --horizon 30 --steps 60 --order --fine > "$OUT/suprof_c4_fine.txt" 2>&1
fi
# the randomised soak at HEAD against the COLD oracle: default mode, the interior-point LamMuZ mode, and - reported, not asserted - the
# opt-in su_tol_early against the oracle at su_tol
timeout 900 python tools/soak.py --scenes 64 --steps 100 --seed 21 --cold > "$OUT/soak_default.txt" 2>&1
timeout 600 python tools/soak.py --scenes 24 --steps 60 --seed 22 --cold --lmz-central 1e-3 > "$OUT/soak_lmz_central.txt" 2>&1
timeout 600 python tools/soak.py --scenes 32 --steps 100 --seed 23 --cold --su-tol-early > "$OUT/soak_su_tol_early.txt" 2>&1
# the scratch tree (raw rocprofv3 output, tens of MB) does not travel back
find "$SCR" -type f -delete
ls -la "$OUT"; head -12 "$OUT/ns_kernel_stats.csv"
