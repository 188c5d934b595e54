#!/bin/bash
# the round's profile set (MI355X): bash tools/prof_final.sh <tag> <out dir>  -> <out dir>/<tag>_* (the step censuses go
# where tools/step_census.sh writes them); a relative <out dir> is taken from the repository root
tag=$1
out=${2:?usage: bash tools/prof_final.sh <tag> <out dir>}
cd "$GRAFT_REPO_ROOT"
mkdir -p "$out"
bash tools/pmc_step.sh "$out/${tag}_pmc" > /dev/null 2>&1
python tools/pmc_hbm_json.py "$out/${tag}_pmc/fetch.txt" "$out/${tag}_pmc/write.txt" --images 16 > "$out/${tag}_trunk_hbm.json"
bash tools/prof_round.sh ${tag} "$out"
python tools/conv_table.py > "$out/${tag}_conv_table.txt" 2> /dev/null
for wl in pix2pix brats cut; do
  bash tools/step_census.sh ${tag}_${wl} $wl > /dev/null 2>&1
done
python bench.py --full > "$out/${tag}_bench.json" 2> "$out/${tag}_bench.err"
tail -c 600 "$out/${tag}_bench.json"
