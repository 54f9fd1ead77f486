#!/bin/bash
# Builds tests/rank_sync_check.cpp (the fold and the barrier of the host-synchronous transports, host code only) with the thread sanitizer and
# with the address + undefined-behaviour sanitizers and runs both on the CPU.  Usage: scripts/rank_sync_sanitize.sh [build dir]
set -euo pipefail
root="$(cd "$(dirname "$0")/.." && pwd)"
out="${1:-$(mktemp -d)}"
for san in thread address,undefined; do
   exe="$out/rank_sync_check_${san%%,*}"
   g++ -std=c++17 -O1 -g -pthread -fsanitize=$san -fno-sanitize-recover=all -o "$exe" "$root/tests/rank_sync_check.cpp"
   echo "-fsanitize=$san:"
   "$exe"
done
