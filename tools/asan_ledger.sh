#!/bin/bash
# The file ledger's host functions under AddressSanitizer + UBSan as a stand-alone program (no GPU, no Python, nothing
# preloaded): tools/asan_ledger_main.cpp linked with hx_xhead.cpp.   bash tools/asan_ledger.sh
set -e
cd "$(dirname "$0")/.."
OUT=$(mktemp -d /tmp/hxasanl.XXXXXX)
trap 'rm -rf "$OUT"' EXIT
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer tools/asan_ledger_main.cpp hmp3_amd/csrc/hx_xhead.cpp -o $OUT/asan_ledger
$OUT/asan_ledger
