#!/bin/bash
# Counters of the denoiser's kernels (k_dn_prep, k_dn_level, k_dn_level_lds) on a filled 1920 x 1080 Cornell frame:
# one rocprofv3 --pmc pass per counter group (never combined with trace domains) over profiles/denoise_rate.py,
# averaged per kernel instantiation into <out>/summary.json (the run of record: profiles/denoise_pmc.json).
#   profiles/denoise_pmc.sh [out directory]
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${1:-$R/bench_out/pmc_dn}; mkdir -p $OUT; export TMPDIR=/tmp
G=("SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT" \
   "SQ_INSTS_VALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS TCC_HIT_sum TCC_MISS_sum")
i=0
for P in "${G[@]}"; do i=$((i+1))
  timeout -k 10 300 rocprofv3 --pmc $P --output-format csv -d $OUT/p$i -o run -- python3 $R/profiles/denoise_rate.py --frames-of 1920x1080 --focals 0.6 > $OUT/p$i.log 2>&1
  rc=$?
  if [ $rc -ne 0 ]; then echo "pass $i failed rc=$rc ($P)"; tail -5 $OUT/p$i.log; exit 1; fi
done
python3 - "$OUT" <<'PY'
import csv, glob, sys, collections, json, re
agg = collections.defaultdict(lambda: collections.defaultdict(list))
for f in sorted(glob.glob(sys.argv[1] + "/p*/**/*counter_collection.csv", recursive=True)):
    for r in csv.DictReader(open(f)):
        if "k_dn_" in r["Kernel_Name"]:
            m = re.search(r"(k_dn_\w+(<[^>]*>)?)", r["Kernel_Name"])
            agg[m.group(1)][r["Counter_Name"]].append(float(r["Counter_Value"]))
out = {k: {c: sum(v) / len(v) for c, v in sorted(d.items())} | {"dispatches": len(next(iter(d.values())))} for k, d in sorted(agg.items())}
json.dump(out, open(sys.argv[1] + "/summary.json", "w"), indent=1)
for k, d in out.items():
    print(k, json.dumps({c: round(v, 1) for c, v in d.items()}))
PY
