#!/bin/bash
# Builds tests/mixed_loading_check.cpp (the step algebra of mixed loading, csrc/host/mixed_loading.hpp, host code only) with the address +
# undefined-behaviour sanitizers and runs it on the CPU.  Usage: scripts/mixed_loading_sanitize.sh [build dir]
set -euo pipefail
root="$(cd "$(dirname "$0")/.." && pwd)"
out="${1:-$(mktemp -d)}"
exe="$out/mixed_loading_check_address"
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o "$exe" "$root/tests/mixed_loading_check.cpp"
echo "-fsanitize=address,undefined:"
"$exe"
