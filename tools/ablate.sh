#!/bin/bash
# timing of the chain kernel of the library that is loaded (development aid).  The timing-only ablations are build variants,
# -DP2S_DEV_ABLATE=<variant> (1 = conv3 only, 2 = all but conv3; of the screened conv3: 3 = its MFMAs and their loads only,
# 4 = everything but the confirm -- its select reads the pool bound E, which then stays -inf --, 5 = everything but the fp16
# conversion of the tile, 7 = variant 4 without the queue loop as well: the whole select, its mask kept by one v_or, 8 = variant 7
# without the mask: column maxima, R and the threshold, kept by one v_max; so per launch mask = 7 - 8, rest of the select = 8 - 3,
# queue = 4 - 7, confirm = shipped - 4 (profiles/r13/select_parts.json); the results of such a build are wrong).  They are values
# of the define, not switches of the library.  There is no variant 6: "no conv0a / conv0b, conv1 fed from
# what is in bufB" was tried for the stem reuse and times nothing -- conv1 reads another layer's output, the screen cannot decide
# and the items re-run densely, three times the shipped launch (profiles/r12/stem_ceiling.json); what the stem costs is the
# difference between a model created with stem_reuse=False and the default (the chain_main figure below).  Build one beside the
# shipped library and point P2S_LIB_PATH at it; this script builds nothing and replaces nothing:
#   P2S_LIB_PATH=/path/to/variant/libp2s_hip.so tools/ablate.sh [queries per launch, default 4096]
python tools/quick_bench.py --B "${1:-4096}" --iters 3 2>/dev/null | tail -1 | python -c '
import sys, json
d = json.loads(sys.stdin.read())
c = d.get("device_clock") or {}
print(round(d["ms"], 2), "ms; chain_stn", round(d["stages_ms"]["ms_chain_stn"], 2), "chain_main", round(d["stages_ms"]["ms_chain_main"], 2),
      "; sclk MHz", round(c.get("sclk_MHz_mean", 0)), "power W", round(c.get("power_W_mean", 0)))'
