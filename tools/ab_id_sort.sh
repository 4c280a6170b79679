#!/bin/bash
# Alternating-process A/B of the id sort's own launch list (csrc/cdr_step.hip, "the id sort's own launch list"), on one GPU:
#   parent   a checkout of the commit before the change, built           (PARENT=<dir>; left out when unset)
#   off      this build, CDR_OWN_SORT=0                                  (the library call; must equal the parent)
#   list     this build, CDR_OWN_SORT=1                                  (own launch list, rocPRIM's histogram and scan launches kept)
#   new      this build as it is                                         (own launch list, key making + histogram + scan in one launch)
# ROUNDS rounds (default 6) of `python bench.py --gpus 1 --steps 30 --warmup 5`, one process per run, arms interleaved; the first round
# also writes --dump-outputs, compared file by file at the end.  Stops at the first run that fails.  Output: OUT (default /tmp/ab_id_sort).
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); O=${OUT:-/tmp/ab_id_sort}; mkdir -p "$O"
run() {
  local name=$1 dir=$2 i=$3; shift 3
  local extra=""; [ "$i" = 1 ] && extra="--dump-outputs $O/dump_$name"
  ( cd "$dir" && env "$@" timeout -k 10 240 python bench.py --gpus 1 --steps 30 --warmup 5 $extra > "$O/${name}_$i.json" 2> "$O/${name}_$i.err" ) \
    || { echo "$name $i failed"; tail -5 "$O/${name}_$i.err"; exit 1; }
  echo "$name $i $(python -c "import json; print('%.4f ms' % json.loads(open('$O/${name}_$i.json').read().strip().splitlines()[-1])['ms_per_step'])")"
}
for i in $(seq 1 "${ROUNDS:-6}"); do
  [ -n "$PARENT" ] && run parent "$PARENT" "$i" CDR_AB=parent
  run off "$R" "$i" CDR_OWN_SORT=0
  run list "$R" "$i" CDR_OWN_SORT=1
  run new "$R" "$i" CDR_AB=new
done
python - "$O" <<'PY'
import glob, json, os, statistics, sys
import numpy as np
O = sys.argv[1]
arms = {}
for f in sorted(glob.glob(os.path.join(O, '*_[0-9]*.json'))):
    arm = os.path.basename(f).rsplit('_', 1)[0]
    arms.setdefault(arm, []).append(json.loads(open(f).read().strip().splitlines()[-1])['ms_per_step'])
out = {a: {'ms_per_step': v, 'median': statistics.median(v), 'min': min(v), 'max': max(v)} for a, v in arms.items()}
ref = 'parent' if 'parent' in arms else 'off'
for other in arms:
    if other == ref:
        continue
    files = sorted(glob.glob(os.path.join(O, 'dump_' + ref, '*.npy')))
    bad = [os.path.basename(f) for f in files if np.load(f).tobytes() != np.load(f.replace('dump_' + ref, 'dump_' + other)).tobytes()]
    out[other]['dump_vs_' + ref] = 'equal (%d files)' % len(files) if files and not bad else 'DIFFER: %s' % bad
    out[other]['every_run_below_every_' + ref + '_run'] = max(arms[other]) < min(arms[ref])
print(json.dumps(out, indent=1))
PY
