#!/bin/sh
# build a differently configured library for A/B runs (loaded through GIPUMA_HIP_LIB under GIPUMA_HIP_EXPERIMENTS=1):
#   sh scripts/build_variant.sh <name> [-DFLAG ...]   ->  gipuma_amd/csrc/variants/libgipuma_hip_<name>.so
# Every translation unit of the product gets the extra flags; the list of them is __graft_entry__.TRANSLATION_UNITS alone.
R=$(cd "$(dirname "$0")/.." && pwd)
cd "$R" && python -c "import sys, __graft_entry__ as g; g.build_variant(sys.argv[1], sys.argv[2:])" "$@"
