#!/bin/bash
# A variant of the library for a same-box A/B (scripts/ab_lib.sh): one unit recompiled with extra defines, the other
# objects taken from build/hip/.  The units, their sources and defines and the objects that are linked are those of
# open_provence_amd/build_ext.py (UNITS): an object left in build/hip/ by an earlier layout of the units is not picked up.
#   usage: scripts/build_variant_lib.sh <name> <unit: row4|row5|attn|panel|api|forward|forward_layers|...> <defines...>
set -eu
cd "$(dirname "$0")/.."
NAME=$1; UNIT=$2; shift 2
mkdir -p ab_libs build/variant
# line 1: object name, source and defines of the unit; line 2: every object of the library, in link order
UNITS=$(python3 - "$UNIT" <<'EOF'
import sys
from open_provence_amd import build_ext
short = lambda name: name.removeprefix("op_launch_").removeprefix("op_")
mine = [u for u in build_ext.UNITS if short(u[0]) == sys.argv[1]]
if not mine:
    sys.exit("unknown unit %s (known: %s)" % (sys.argv[1], " ".join(short(u[0]) for u in build_ext.UNITS)))
print(mine[0][0], mine[0][1], *mine[0][2])
print(*[u[0] for u in build_ext.UNITS])
EOF
)
read -r OBJ SRC PART <<<"$(sed -n 1p <<<"$UNITS")"
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result -fno-slp-vectorize $PART "$@" -c $SRC -o build/variant/${NAME}_$OBJ.o
OBJS=""
for b in $(sed -n 2p <<<"$UNITS"); do
  if [ "$b" = "$OBJ" ]; then OBJS="$OBJS build/variant/${NAME}_$OBJ.o"; else OBJS="$OBJS build/hip/$b.o"; fi
done
hipcc --offload-arch=gfx950 -shared -fPIC -o ab_libs/$NAME.so $OBJS
ls -la ab_libs/$NAME.so
