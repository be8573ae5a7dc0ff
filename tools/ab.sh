# usage: ab.sh "ENV1" "ENV2" ...   (each a space-separated env assignment list; "-" = none)
T=$(mktemp -d)
for e in "$@"; do
  if [ "$e" = "-" ]; then e=""; fi
  env $e python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-aux > $T/ab.json 2>$T/ab.err
  python -c "
import json,sys; d=json.load(open(sys.argv[2])); print(sys.argv[1] or '-', d['ms_per_step'], d['config']['encode_ms'], d['config']['decode_ms'], d['roofline']['achieved'])" "$e" $T/ab.json || tail -3 $T/ab.err
done
rm -rf $T
