# Build diagnostic kernel variants for scripts/ab_probe.py and the other probes:
# build/libraftsim_<name>.so with extra -D flags (csrc/device.hpp lists the switches). Every variant
# is a RS_DIAG_BUILD: tagged "diag", refused by raftsim.check_build, loaded through RAFTSIM_LIB.
# The command is the product's (raftsim/_build.py: variant_command), so a variant links what the
# product links.
# Usage: bash scripts/build_variants.sh name1 "-DFLAG=1 ..." name2 "..." ...
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$R/raft-simulation_amd/build"
exec python3 - "$R" "$@" <<'PY'
import subprocess, sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

root, args = Path(sys.argv[1]), sys.argv[2:]
sys.path.insert(0, str(root / "raft-simulation_amd"))
from raftsim import _build

JOBS = 16        # concurrent compiles at most
cmds = [_build.variant_command(root / f"raft-simulation_amd/build/libraftsim_{name}.so",
                               flags.split(), root)
        for name, flags in zip(args[::2], args[1::2])]
with ThreadPoolExecutor(JOBS) as pool:
    codes = list(pool.map(lambda c: subprocess.run(c).returncode, cmds))
sys.exit(1 if any(codes) else 0)     # a failed variant fails the script
PY
