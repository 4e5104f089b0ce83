#!/bin/bash
# Builds tests/cpp/records_found_fuzz.cpp — the host path of decrypt_strings (aleo_amd/csrc/records_found_host.hpp) and the lane functions it shares with the
# kernels — with the host-only translation units it needs (wire.hip: the record parser and bech32m; sponge.hip: Poseidon) as plain C++ under AddressSanitizer +
# UndefinedBehaviorSanitizer, and runs it.  A program of its own: no GPU, no HIP runtime, nothing loaded into another process.
# Usage: tools/asan_records_found.sh <out dir> <case file> <view key hex> <address x hex>
set -euo pipefail
root="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"; out="$1"; mkdir -p "$out"
CXXF="-std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -mbmi2 -madx -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I$root/include"
printf '#include <string>\nnamespace aleo_mi355x { thread_local std::string g_last_error; }\nextern "C" const char* aleo_mi355x_last_error(void) { return aleo_mi355x::g_last_error.c_str(); }\n' > "$out/stub.cpp"
g++ $CXXF -x c++ -c "$root/aleo_amd/csrc/wire.hip" -o "$out/wire.o" &
g++ $CXXF -x c++ -c "$root/aleo_amd/csrc/sponge.hip" -o "$out/sponge.o" &
g++ $CXXF -c "$out/stub.cpp" -o "$out/stub.o" &
g++ $CXXF -c "$root/tests/cpp/records_found_fuzz.cpp" -o "$out/records_found_fuzz.o" &
wait
g++ -fsanitize=address,undefined "$out/wire.o" "$out/sponge.o" "$out/stub.o" "$out/records_found_fuzz.o" -o "$out/records_found_fuzz"
ASAN_OPTIONS=detect_leaks=1:abort_on_error=0 UBSAN_OPTIONS=print_stacktrace=1 "$out/records_found_fuzz" "$2" "$3" "$4"
