#!/bin/bash
# tools/ar_driver_rules_check.sh: the AR request driver's host rules (csrc/ar_rules.cpp) under AddressSanitizer + UBSan, as a stand-alone program on the CPU.
# Host code only: nothing here opens a device.
cd "$(dirname "$0")/../tortoise.cpp_amd" || exit 1
mkdir -p ../tools/bin
/opt/rocm/bin/hipcc -O1 -g -std=c++17 -x hip --offload-host-only -Wall -Wno-unused-result -Icsrc -I../include \
  -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
  ../tools/ar_driver_rules_check.cpp csrc/ar_rules.cpp csrc/host_logic.cpp -o ../tools/bin/ar_driver_rules_check || exit 1
exec ../tools/bin/ar_driver_rules_check
