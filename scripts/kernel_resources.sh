# Registers, scratch and occupancy of every kernel of every compiled unit, as the compiler reports
# them, written to profiles/TAG_kernel_resources.txt. Compiles only; scripts/kernel_asm.py does the
# work, and also compares two trees' device assembly kernel by kernel.
# Usage: bash scripts/kernel_resources.sh TAG
set -e
TAG=${1:-r12}
R=$(cd "$(dirname "$0")/.." && pwd)
python3 "$R/scripts/kernel_asm.py" > "$R/profiles/${TAG}_kernel_resources.txt"
cat "$R/profiles/${TAG}_kernel_resources.txt"
