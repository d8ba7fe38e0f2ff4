#!/bin/bash
# builds scripts/probes/lane_priority.hip if its binary is missing and runs it once under a time limit; the output is what profiles/lane_priority_probe.md quotes
set -u
cd "$(dirname "$0")/../.."
if [ ! -x scripts/probes/lane_priority_probe ]; then
  hipcc --offload-arch=gfx950 -O2 scripts/probes/lane_priority.hip -o scripts/probes/lane_priority_probe || exit 1
fi
timeout -k 10 120 scripts/probes/lane_priority_probe
