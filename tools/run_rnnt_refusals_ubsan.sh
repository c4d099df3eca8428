#!/bin/bash
# Build tools/rnnt_refusals_ubsan.cc with the host side of the sources it links against under the
# undefined-behaviour sanitizer, and run it.  No device is needed; nothing is loaded into Python.
#     tools/run_rnnt_refusals_ubsan.sh [directory for the program, default a temporary one]
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${1:-$(mktemp -d)}"
CS="$ROOT/speech2text_amd/csrc"
"${HIPCC:-/opt/rocm/bin/hipcc}" -O1 -std=c++17 --offload-arch=gfx950 -fno-gpu-rdc -fPIC -I"$ROOT/include" \
  -Xarch_host -fsanitize=undefined -Xarch_host -fno-sanitize-recover=undefined \
  "$ROOT/tools/rnnt_refusals_ubsan.cc" "$CS/decode_rnnt.hip" "$CS/decode.hip" "$CS/decode_lstm.hip" "$CS/ngram.hip" \
  -o "$OUT/rnnt_refusals_ubsan"
"$OUT/rnnt_refusals_ubsan"
