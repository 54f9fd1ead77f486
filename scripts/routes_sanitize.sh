#!/bin/bash
# Builds tests/routes_check.cpp (the operator's switches, route decision and cap choosers of csrc/host/routes.cpp, host code only) with the
# address + undefined-behaviour sanitizers and runs it on the CPU.  Usage: scripts/routes_sanitize.sh [build dir]
set -euo pipefail
root="$(cd "$(dirname "$0")/.." && pwd)"
out="${1:-$(mktemp -d)}"
exe="$out/routes_check_address"
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o "$exe" "$root/tests/routes_check.cpp"
echo "-fsanitize=address,undefined:"
"$exe"
