"""The refusals of the analyses' Python layer (stringdecomposer_amd/lib.py: --lags, --heatmap, --autocorr, --motif, --dotplot,
--split, --hor, --msa, --profile) that are raised before a device is needed, and the one-line refusals of the command line's
checks (stringdecomposer_amd/main.py): SdError.code and the whole SdError.msg, the whole stderr line and the exit code, case by
case.  The texts are what the layer said when every analysis still carried its own copy of these checks, taken from a run of
that commit.  The *_device entry points check their integers before they import torch, so their refusals are here too."""
import argparse

import numpy as np
import pytest

from stringdecomposer_amd import lib
from stringdecomposer_amd import main as sdmain

PARAM = lib.SD_ERR_PARAM
TEXT = b"ACGTACGTACGTACGT"
ST, EN, GO = [0, 4], [3, 7], [0, 2]
MONOS = [b"ACGTACGT"]
SYM = np.zeros((4, 8), dtype=np.uint8)
BIG = 1 << 63
OUTSIDE = "offsets and lengths differ in number, or a read lies outside the text"
PCT = "must be an integer 1 .. 100 (a percentage of the monomer's length)"


def rows_of(*reads):
    rows = np.zeros(len(reads), dtype=lib.final_dtype())
    rows["read"] = reads
    return (rows, None, None)


# name -> (call, text); every case is SD_ERR_PARAM
CASES = {
    # ---- lags: 1 <= D <= 255 ----
    "lag_segments D=0": (lambda: lib.lag_segments(TEXT, ST, EN, GO, 0), "lag_segments: D = 0, must be an integer 1 .. 255"),
    "lag_segments D=256": (lambda: lib.lag_segments(TEXT, ST, EN, GO, 256), "lag_segments: D = 256, must be an integer 1 .. 255"),
    "lag_segments D=2.0": (lambda: lib.lag_segments(TEXT, ST, EN, GO, 2.0), "lag_segments: D = 2.0, must be an integer 1 .. 255"),
    "lag_segments D=True": (lambda: lib.lag_segments(TEXT, ST, EN, GO, True), "lag_segments: D = True, must be an integer 1 .. 255"),
    "lag_segments ends short": (lambda: lib.lag_segments(TEXT, ST, [3], GO, 2),
                                "lag_segments: starts and ends differ in length, or group_off is empty"),
    "lag_segments no group_off": (lambda: lib.lag_segments(TEXT, ST, EN, [], 2),
                                  "lag_segments: starts and ends differ in length, or group_off is empty"),
    "lag_segments group_off 2-D": (lambda: lib.lag_segments(TEXT, ST, EN, [[0, 2]], 2),
                                   "lag_segments: starts and ends differ in length, or group_off is empty"),
    "lag_segments D=0, ends short": (lambda: lib.lag_segments(TEXT, ST, [3], GO, 0), "lag_segments: D = 0, must be an integer 1 .. 255"),
    "lag_kernel_bench D=0": (lambda: lib.lag_kernel_bench(TEXT, ST, EN, GO, 0), "lag_kernel_bench: D = 0, must be an integer 1 .. 255"),
    "lag_kernel_bench D=True": (lambda: lib.lag_kernel_bench(TEXT, ST, EN, GO, True),
                                "lag_kernel_bench: D = True, must be an integer 1 .. 255"),
    "final_lags_device D=0": (lambda: lib.final_lags_device(None, None, 0), "final_lags_device: D = 0, must be an integer 1 .. 255"),
    "final_lags_device D=True": (lambda: lib.final_lags_device(None, None, True),
                                 "final_lags_device: D = True, must be an integer 1 .. 255"),
    "final_lags_host D=256": (lambda: lib.final_lags_host(None, None, 256), "final_lags_host: D = 256, must be an integer 1 .. 255"),
    "final_lags_host D=True": (lambda: lib.final_lags_host(None, None, True), "final_lags_host: D = True, must be an integer 1 .. 255"),
    # ---- heatmap: 1 <= B <= 2^20, W >= 0, max_pairs >= 0 ----
    "heat_layout B=0": (lambda: lib.heat_layout(GO, 0), "heat_layout: B = 0, must be an integer 1 .. 1048576"),
    "heat_layout B=True": (lambda: lib.heat_layout(GO, True), "heat_layout: B = True, must be an integer 1 .. 1048576"),
    "heat_layout W=-1": (lambda: lib.heat_layout(GO, 2, -1), "heat_layout: W = -1, must be an integer, 0 (no limit) or more"),
    "heat_layout W=True": (lambda: lib.heat_layout(GO, 2, True), "heat_layout: W = True, must be an integer, 0 (no limit) or more"),
    "heat_layout no group_off": (lambda: lib.heat_layout([], 2), "heat_layout: group_off is empty"),
    "heat_layout B=0, W=-1": (lambda: lib.heat_layout(GO, 0, -1), "heat_layout: B = 0, must be an integer 1 .. 1048576"),
    "heat_layout B=0, no group_off": (lambda: lib.heat_layout([], 0), "heat_layout: B = 0, must be an integer 1 .. 1048576"),
    "heat_segments B=2^20+1": (lambda: lib.heat_segments(TEXT, ST, EN, GO, (1 << 20) + 1),
                               "heat_segments: B = 1048577, must be an integer 1 .. 1048576"),
    "heat_segments B=True": (lambda: lib.heat_segments(TEXT, ST, EN, GO, True), "heat_segments: B = True, must be an integer 1 .. 1048576"),
    "heat_segments W=2^62": (lambda: lib.heat_segments(TEXT, ST, EN, GO, 2, 1 << 62),
                             "heat_segments: W = 4611686018427387904, must be an integer, 0 (no limit) or more"),
    "heat_segments W=True": (lambda: lib.heat_segments(TEXT, ST, EN, GO, 2, True),
                             "heat_segments: W = True, must be an integer, 0 (no limit) or more"),
    "heat_segments max_pairs=-1": (lambda: lib.heat_segments(TEXT, ST, EN, GO, 2, max_pairs=-1),
                                   "heat_segments: max_pairs = -1, must be an integer, 0 (no limit) or more"),
    "heat_segments max_pairs=1.5": (lambda: lib.heat_segments(TEXT, ST, EN, GO, 2, max_pairs=1.5),
                                    "heat_segments: max_pairs = 1.5, must be an integer, 0 (no limit) or more"),
    "heat_segments max_pairs=True": (lambda: lib.heat_segments(TEXT, ST, EN, GO, 2, max_pairs=True),
                                     "heat_segments: max_pairs = True, must be an integer, 0 (no limit) or more"),
    "heat_segments ends short": (lambda: lib.heat_segments(TEXT, ST, [3], GO, 2),
                                 "heat_segments: starts and ends differ in length, or group_off is empty"),
    "heat_segments no group_off": (lambda: lib.heat_segments(TEXT, ST, EN, [], 2),
                                   "heat_segments: starts and ends differ in length, or group_off is empty"),
    "heat_segments W=-1, ends short": (lambda: lib.heat_segments(TEXT, ST, [3], GO, 2, -1),
                                       "heat_segments: W = -1, must be an integer, 0 (no limit) or more"),
    "heat_kernel_bench B=0": (lambda: lib.heat_kernel_bench(TEXT, ST, EN, GO, 0), "heat_kernel_bench: B = 0, must be an integer 1 .. 1048576"),
    "heat_kernel_bench W=True": (lambda: lib.heat_kernel_bench(TEXT, ST, EN, GO, 2, True),
                                 "heat_kernel_bench: W = True, must be an integer, 0 (no limit) or more"),
    "heat_kernel_bench B=0, W=True": (lambda: lib.heat_kernel_bench(TEXT, ST, EN, GO, 0, True),
                                      "heat_kernel_bench: B = 0, must be an integer 1 .. 1048576"),
    "final_heat_device B=0": (lambda: lib.final_heat_device(None, None, 0), "final_heat_device: B = 0, must be an integer 1 .. 1048576"),
    "final_heat_device B=True": (lambda: lib.final_heat_device(None, None, True),
                                 "final_heat_device: B = True, must be an integer 1 .. 1048576"),
    "final_heat_device W=-1": (lambda: lib.final_heat_device(None, None, 2, -1),
                               "final_heat_device: W = -1, must be an integer, 0 (no limit) or more"),
    "final_heat_device max_pairs=True": (lambda: lib.final_heat_device(None, None, 2, max_pairs=True),
                                         "final_heat_device: max_pairs = True, must be an integer, 0 (no limit) or more"),
    "final_heat_device B=0, max_pairs=-1": (lambda: lib.final_heat_device(None, None, 0, max_pairs=-1),
                                            "final_heat_device: B = 0, must be an integer 1 .. 1048576"),
    "final_heat_host B=0": (lambda: lib.final_heat_host(None, None, 0), "final_heat_host: B = 0, must be an integer 1 .. 1048576"),
    "final_heat_host W=True": (lambda: lib.final_heat_host(None, None, 2, True),
                               "final_heat_host: W = True, must be an integer, 0 (no limit) or more"),
    "final_heat_host max_pairs=-1": (lambda: lib.final_heat_host(None, None, 2, max_pairs=-1),
                                     "final_heat_host: max_pairs = -1, must be an integer, 0 (no limit) or more"),
    "final_heat_host a row of no read": (lambda: lib.final_heat_host(rows_of(0, 2), [TEXT], 2),
                                         "final_heat_host: a row's read index lies outside the 1 reads"),
    "final_heat_host B=0, a row of no read": (lambda: lib.final_heat_host(rows_of(0, 2), [TEXT], 0),
                                              "final_heat_host: B = 0, must be an integer 1 .. 1048576"),
    "final_heat_host max_pairs=-1, a row of no read": (lambda: lib.final_heat_host(rows_of(0, 2), [TEXT], 2, max_pairs=-1),
                                                       "final_heat_host: max_pairs = -1, must be an integer, 0 (no limit) or more"),
    # ---- autocorr: 1 <= k <= 32, 1 <= D <= 2^20, window >= 0 ----
    "autocorr_layout window=-1": (lambda: lib.autocorr_layout([10], -1),
                                  "autocorr_layout: window = -1, must be an integer, 0 (one window) or more"),
    "autocorr_layout window=True": (lambda: lib.autocorr_layout([10], True),
                                    "autocorr_layout: window = True, must be an integer, 0 (one window) or more"),
    "autocorr k=0": (lambda: lib.autocorr([TEXT], 0), "autocorr: k = 0, must be an integer 1 .. 32"),
    "autocorr k=33": (lambda: lib.autocorr([TEXT], 33), "autocorr: k = 33, must be an integer 1 .. 32"),
    "autocorr k=True": (lambda: lib.autocorr([TEXT], True), "autocorr: k = True, must be an integer 1 .. 32"),
    "autocorr D=0": (lambda: lib.autocorr([TEXT], 4, 0), "autocorr: D = 0, must be an integer 1 .. 1048576"),
    "autocorr D=True": (lambda: lib.autocorr([TEXT], 4, True), "autocorr: D = True, must be an integer 1 .. 1048576"),
    "autocorr window=4.0": (lambda: lib.autocorr([TEXT], 4, 8, 4.0), "autocorr: window = 4.0, must be an integer, 0 (one window) or more"),
    "autocorr window=True": (lambda: lib.autocorr([TEXT], 4, 8, True), "autocorr: window = True, must be an integer, 0 (one window) or more"),
    "autocorr k=0, D=0": (lambda: lib.autocorr([TEXT], 0, 0), "autocorr: k = 0, must be an integer 1 .. 32"),
    "autocorr_text k=0": (lambda: lib.autocorr_text(TEXT, [0], [16], 0), "autocorr: k = 0, must be an integer 1 .. 32"),
    "autocorr_text past the text": (lambda: lib.autocorr_text(TEXT, [0], [17], 4), "autocorr: " + OUTSIDE),
    "autocorr_text negative offset": (lambda: lib.autocorr_text(TEXT, [-1], [4], 4), "autocorr: " + OUTSIDE),
    "autocorr_text negative length": (lambda: lib.autocorr_text(TEXT, [0], [-1], 4), "autocorr: " + OUTSIDE),
    "autocorr_text two offsets, one length": (lambda: lib.autocorr_text(TEXT, [0, 4], [4], 4), "autocorr: " + OUTSIDE),
    "autocorr_text D=0, past the text": (lambda: lib.autocorr_text(TEXT, [0], [17], 4, 0), "autocorr: D = 0, must be an integer 1 .. 1048576"),
    "autocorr_device k=0": (lambda: lib.autocorr_device(None, 0), "autocorr_device: k = 0, must be an integer 1 .. 32"),
    "autocorr_device k=True": (lambda: lib.autocorr_device(None, True), "autocorr_device: k = True, must be an integer 1 .. 32"),
    "autocorr_device D=2^20+1": (lambda: lib.autocorr_device(None, 4, (1 << 20) + 1),
                                 "autocorr_device: D = 1048577, must be an integer 1 .. 1048576"),
    "autocorr_device window=-1": (lambda: lib.autocorr_device(None, 4, 8, -1),
                                  "autocorr_device: window = -1, must be an integer, 0 (one window) or more"),
    "autocorr_device k=0, D=0": (lambda: lib.autocorr_device(None, 0, 0), "autocorr_device: k = 0, must be an integer 1 .. 32"),
    "autocorr_device D=0, window=-1": (lambda: lib.autocorr_device(None, 4, 0, -1), "autocorr_device: D = 0, must be an integer 1 .. 1048576"),
    "autocorr_positions k=0": (lambda: lib.autocorr_positions([10], 0, 4), "autocorr_positions: k = 0, must be an integer 1 .. 32"),
    "autocorr_positions D=True": (lambda: lib.autocorr_positions([10], 4, True), "autocorr_positions: D = True, must be an integer 1 .. 1048576"),
    "autocorr_positions over the cap": (lambda: lib.autocorr_positions([1] * 129, 4, 1 << 20),
                                        "autocorr_positions: 129 windows x 1048576 lags, the cap is 134217728 cells"),
    "autocorr_positions k=0, over the cap": (lambda: lib.autocorr_positions([1] * 129, 0, 1 << 20),
                                             "autocorr_positions: k = 0, must be an integer 1 .. 32"),
    "autocorr_positions D=2^20+1, over the cap": (lambda: lib.autocorr_positions([1] * 129, 4, (1 << 20) + 1),
                                                  "autocorr_positions: D = 1048577, must be an integer 1 .. 1048576"),
    "autocorr_positions window=-1, over the cap": (lambda: lib.autocorr_positions([1] * 129, 4, 1 << 20, -1),
                                                   "autocorr_positions: window = -1, must be an integer, 0 (one window) or more"),
    "autocorr_seed k=0": (lambda: lib.autocorr_seed(TEXT, 0, 4), "autocorr_seed: k = 0, must be an integer 1 .. 32"),
    "autocorr_seed k=True": (lambda: lib.autocorr_seed(TEXT, True, 4), "autocorr_seed: k = True, must be an integer 1 .. 32"),
    "autocorr_seed p=0": (lambda: lib.autocorr_seed(TEXT, 2, 0), "autocorr_seed: p = 0, must be an integer, 1 or more"),
    "autocorr_seed p=4.0": (lambda: lib.autocorr_seed(TEXT, 2, 4.0), "autocorr_seed: p = 4.0, must be an integer, 1 or more"),
    "autocorr_seed k=0, p=0": (lambda: lib.autocorr_seed(TEXT, 0, 0), "autocorr_seed: k = 0, must be an integer 1 .. 32"),
    "autocorr_kernel_bench k=0": (lambda: lib.autocorr_kernel_bench([TEXT], 0), "autocorr_kernel_bench: k = 0, must be an integer 1 .. 32"),
    "autocorr_kernel_bench window=True": (lambda: lib.autocorr_kernel_bench([TEXT], 4, 8, True),
                                          "autocorr_kernel_bench: window = True, must be an integer, 0 (one window) or more"),
    "autocorr_kernel_bench k=0, D=0": (lambda: lib.autocorr_kernel_bench([TEXT], 0, 0), "autocorr_kernel_bench: k = 0, must be an integer 1 .. 32"),
    "autocorr_peaks lo=0": (lambda: lib.autocorr_peaks([[1, 2]], 0), "autocorr_peaks: lo = 0, must be an integer, 1 or more"),
    "autocorr_peaks lo=True": (lambda: lib.autocorr_peaks([[1, 2]], True), "autocorr_peaks: lo = True, must be an integer, 1 or more"),
    "autocorr_peaks lo=2^31": (lambda: lib.autocorr_peaks([[1, 2]], 1 << 31), "autocorr_peaks: lo = 2147483648, must be an integer, 1 or more"),
    "autocorr_peaks radius=-1": (lambda: lib.autocorr_peaks([[1, 2]], 1, -1), "autocorr_peaks: radius = -1, must be an integer, 0 or more"),
    "autocorr_peaks radius=True": (lambda: lib.autocorr_peaks([[1, 2]], 1, True), "autocorr_peaks: radius = True, must be an integer, 0 or more"),
    "autocorr_peaks peaks=1.5": (lambda: lib.autocorr_peaks([[1, 2]], 1, 8, 1.5), "autocorr_peaks: peaks = 1.5, must be an integer, 0 or more"),
    "autocorr_peaks peaks=True": (lambda: lib.autocorr_peaks([[1, 2]], 1, 8, True), "autocorr_peaks: peaks = True, must be an integer, 0 or more"),
    "autocorr_peaks counts 3-D": (lambda: lib.autocorr_peaks([[[1, 2]]]), "autocorr_peaks: counts must be [windows, D] with 1 <= D <= 1048576"),
    "autocorr_peaks counts D=0": (lambda: lib.autocorr_peaks([[]]), "autocorr_peaks: counts must be [windows, D] with 1 <= D <= 1048576"),
    "autocorr_peaks lo=0, counts 3-D": (lambda: lib.autocorr_peaks([[[1, 2]]], 0), "autocorr_peaks: lo = 0, must be an integer, 1 or more"),
    # ---- motif: the mismatches fit an int32 (the range is the library's to refuse) ----
    "motif_request unknown name": (lambda: lib.motif_request(["nosuch"]),
                                   "motif 'nosuch' is neither NAME=PATTERN nor one of the built-in motifs (cenpb)"),
    "motif_compile E=1.5": (lambda: lib.motif_compile(["cenpb"], 1.5), "motif_compile: mismatches = 1.5, must be an integer 0 .. 7"),
    "motif_compile E=True": (lambda: lib.motif_compile(["cenpb"], True), "motif_compile: mismatches = True, must be an integer 0 .. 7"),
    "motif_compile E=2^31": (lambda: lib.motif_compile(["cenpb"], 1 << 31),
                             "motif_compile: mismatches = 2147483648, must be an integer 0 .. 7"),
    "motif_compile unknown name, E=1.5": (lambda: lib.motif_compile(["nosuch"], 1.5),
                                          "motif 'nosuch' is neither NAME=PATTERN nor one of the built-in motifs (cenpb)"),
    "motif E=True": (lambda: lib.motif([TEXT], ["cenpb"], True), "motif_compile: mismatches = True, must be an integer 0 .. 7"),
    "motif unknown name, E=True": (lambda: lib.motif([TEXT], ["nosuch"], True),
                                   "motif 'nosuch' is neither NAME=PATTERN nor one of the built-in motifs (cenpb)"),
    "motif_text E=1.5": (lambda: lib.motif_text(TEXT, [0], [16], ["cenpb"], 1.5), "motif_compile: mismatches = 1.5, must be an integer 0 .. 7"),
    "motif_text past the text": (lambda: lib.motif_text(TEXT, [0], [17], ["cenpb"]), "motif: " + OUTSIDE),
    "motif_text two offsets, one length": (lambda: lib.motif_text(TEXT, [0, 4], [4], ["cenpb"]), "motif: " + OUTSIDE),
    "motif_text E=True, past the text": (lambda: lib.motif_text(TEXT, [0], [17], ["cenpb"], True),
                                         "motif_compile: mismatches = True, must be an integer 0 .. 7"),
    "motif_device E=1.5": (lambda: lib.motif_device(None, ["cenpb"], 1.5), "motif_compile: mismatches = 1.5, must be an integer 0 .. 7"),
    "motif_device E=True": (lambda: lib.motif_device(None, ["cenpb"], True), "motif_compile: mismatches = True, must be an integer 0 .. 7"),
    "motif_kernel_bench E=1.5": (lambda: lib.motif_kernel_bench([TEXT], ["cenpb"], 1.5),
                                 "motif_compile: mismatches = 1.5, must be an integer 0 .. 7"),
    "motif_device unknown name, E=1.5": (lambda: lib.motif_device(None, ["nosuch"], 1.5),
                                         "motif 'nosuch' is neither NAME=PATTERN nor one of the built-in motifs (cenpb)"),
    "motif_kernel_bench unknown name, E=True": (lambda: lib.motif_kernel_bench([TEXT], ["nosuch"], True),
                                                "motif 'nosuch' is neither NAME=PATTERN nor one of the built-in motifs (cenpb)"),
    # ---- dotplot: 1 <= k <= 32, 1 <= W <= 2^30, 0 <= B <= 2^30, 1 <= M <= 2^20 ----
    "dotplot_layout W=0": (lambda: lib.dotplot_layout([10], 0), "dotplot_layout: W = 0, must be an integer 1 .. 1073741824"),
    "dotplot_layout W=True": (lambda: lib.dotplot_layout([10], True), "dotplot_layout: W = True, must be an integer 1 .. 1073741824"),
    "dotplot_layout B=-1": (lambda: lib.dotplot_layout([10], 4, -1), "dotplot_layout: B = -1, must be an integer 0 .. 1073741824"),
    "dotplot_layout W=0, B=-1": (lambda: lib.dotplot_layout([10], 0, -1), "dotplot_layout: W = 0, must be an integer 1 .. 1073741824"),
    "dotplot k=0": (lambda: lib.dotplot([TEXT], 0, 4), "dotplot: k = 0, must be an integer 1 .. 32"),
    "dotplot k=True": (lambda: lib.dotplot([TEXT], True, 4), "dotplot: k = True, must be an integer 1 .. 32"),
    "dotplot W=2^30+1": (lambda: lib.dotplot([TEXT], 4, (1 << 30) + 1), "dotplot: W = 1073741825, must be an integer 1 .. 1073741824"),
    "dotplot W=True": (lambda: lib.dotplot([TEXT], 4, True), "dotplot: W = True, must be an integer 1 .. 1073741824"),
    "dotplot B=True": (lambda: lib.dotplot([TEXT], 4, 4, True), "dotplot: B = True, must be an integer 0 .. 1073741824"),
    "dotplot M=0": (lambda: lib.dotplot([TEXT], 4, 4, 0, 0), "dotplot: M = 0, must be an integer 1 .. 1048576"),
    "dotplot M=True": (lambda: lib.dotplot([TEXT], 4, 4, 0, True), "dotplot: M = True, must be an integer 1 .. 1048576"),
    "dotplot k=0, M=0": (lambda: lib.dotplot([TEXT], 0, 4, 0, 0), "dotplot: k = 0, must be an integer 1 .. 32"),
    "dotplot_text W=0": (lambda: lib.dotplot_text(TEXT, [0], [16], 4, 0), "dotplot: W = 0, must be an integer 1 .. 1073741824"),
    "dotplot_text past the text": (lambda: lib.dotplot_text(TEXT, [0], [17], 4, 4), "dotplot: " + OUTSIDE),
    "dotplot_text two offsets, one length": (lambda: lib.dotplot_text(TEXT, [0, 4], [4], 4, 4), "dotplot: " + OUTSIDE),
    "dotplot_text W=0, past the text": (lambda: lib.dotplot_text(TEXT, [0], [17], 4, 0), "dotplot: W = 0, must be an integer 1 .. 1073741824"),
    "dotplot_text over the cap": (lambda: lib.dotplot_text(b"A" * 16385, [0], [16385], 4, 1),
                                  "dotplot: 16385 windows make 134242305 cells, the cap is 134217728 (SD_DOTPLOT_CELLS_MAX): use longer "
                                  "windows, a band or fewer reads per call"),
    "dotplot_device k=0": (lambda: lib.dotplot_device([TEXT], 0, 4), "dotplot_device: k = 0, must be an integer 1 .. 32"),
    "dotplot_device W=True": (lambda: lib.dotplot_device([TEXT], 4, True), "dotplot_device: W = True, must be an integer 1 .. 1073741824"),
    "dotplot_device M=2^20+1": (lambda: lib.dotplot_device(None, 4, 4, 0, (1 << 20) + 1),
                                "dotplot_device: M = 1048577, must be an integer 1 .. 1048576"),
    "dotplot_device k=0, M=0": (lambda: lib.dotplot_device([TEXT], 0, 4, 0, 0), "dotplot_device: k = 0, must be an integer 1 .. 32"),
    "dotplot_device W=0, B=-1": (lambda: lib.dotplot_device(None, 4, 0, -1), "dotplot_device: W = 0, must be an integer 1 .. 1073741824"),
    "dotplot_kernel_bench k=0": (lambda: lib.dotplot_kernel_bench([TEXT], 0, 4), "dotplot_kernel_bench: k = 0, must be an integer 1 .. 32"),
    "dotplot_kernel_bench B=True": (lambda: lib.dotplot_kernel_bench([TEXT], 4, 4, True),
                                    "dotplot_kernel_bench: B = True, must be an integer 0 .. 1073741824"),
    "dotplot_kernel_bench k=0, W=0": (lambda: lib.dotplot_kernel_bench([TEXT], 0, 0), "dotplot_kernel_bench: k = 0, must be an integer 1 .. 32"),
    # ---- split: R, min_size, max_iter >= 1, 1 <= K <= 64, 1 <= P <= 100 ----
    "split_rows R=0": (lambda: lib.split_rows(SYM, 0), "split_rows: R = 0, must be an integer, 1 or more"),
    "split_rows R=1.0": (lambda: lib.split_rows(SYM, 1.0), "split_rows: R = 1.0, must be an integer, 1 or more"),
    "split_rows R=True": (lambda: lib.split_rows(SYM, True), "split_rows: R = True, must be an integer, 1 or more"),
    "split_rows R=2^31": (lambda: lib.split_rows(SYM, 1 << 31), "split_rows: R = 2147483648, must be an integer, 1 or more"),
    "split_rows K=65": (lambda: lib.split_rows(SYM, 2, 65), "split_rows: K = 65, must be an integer 1 .. 64"),
    "split_rows K=True": (lambda: lib.split_rows(SYM, 2, True), "split_rows: K = True, must be an integer 1 .. 64"),
    "split_rows min_size=0": (lambda: lib.split_rows(SYM, 2, 4, 0), "split_rows: min_size = 0, must be an integer, 1 or more"),
    "split_rows min_size=True": (lambda: lib.split_rows(SYM, 2, 4, True), "split_rows: min_size = True, must be an integer, 1 or more"),
    "split_rows max_iter=0": (lambda: lib.split_rows(SYM, 2, 4, 2, 0), "split_rows: max_iter = 0, must be an integer, 1 or more"),
    "split_rows max_iter=True": (lambda: lib.split_rows(SYM, 2, 4, 2, True), "split_rows: max_iter = True, must be an integer, 1 or more"),
    "split_rows K=0, min_size=0": (lambda: lib.split_rows(SYM, 2, 0, 0), "split_rows: min_size = 0, must be an integer, 1 or more"),
    "split_rows sym 1-D": (lambda: lib.split_rows([0, 1, 2], 2), "split_rows: sym must be [n, L] with L >= 1"),
    "split_rows a symbol above 5": (lambda: lib.split_rows(SYM + 6, 2), "split_rows: a symbol above 5 (0..4 = A C G T N, 5 = deleted)"),
    "split_rows R=0, sym 1-D": (lambda: lib.split_rows([0, 1, 2], 0), "split_rows: R = 0, must be an integer, 1 or more"),
    "split_msa P=0": (lambda: lib.split_msa(None, [], [], 0), "split_msa: P = 0, " + PCT),
    "split_msa P=101": (lambda: lib.split_msa(None, [], [], 101), "split_msa: P = 101, " + PCT),
    "split_msa P=True": (lambda: lib.split_msa(None, [], [], True), "split_msa: P = True, " + PCT),
    "split_msa P=15.0": (lambda: lib.split_msa(None, [], [], 15.0), "split_msa: P = 15.0, " + PCT),
    "split_msa K=0": (lambda: lib.split_msa(None, [], [], 15, 0), "split_msa: K = 0, must be an integer 1 .. 64"),
    "split_msa max_iter=True": (lambda: lib.split_msa(None, [], [], 15, 4, 2, True), "split_msa: max_iter = True, must be an integer, 1 or more"),
    "split_msa P=0, K=0": (lambda: lib.split_msa(None, [], [], 0, 0), "split_msa: P = 0, " + PCT),
    "final_split_host P=0": (lambda: lib.final_split_host(None, [], [8], 0), "final_split_host: P = 0, " + PCT),
    "final_split_host P=True": (lambda: lib.final_split_host(None, [], [8], True), "final_split_host: P = True, " + PCT),
    "final_split_host K=65": (lambda: lib.final_split_host(None, [], [8], 15, 65), "final_split_host: K = 65, must be an integer 1 .. 64"),
    "final_split_host min_size=True": (lambda: lib.final_split_host(None, [], [8], 15, 4, True),
                                       "final_split_host: min_size = True, must be an integer, 1 or more"),
    "final_split_host an empty monomer": (lambda: lib.final_split_host(None, [], [8, 0], 15), "final_split_host: an empty monomer"),
    "final_split_host P=101, an empty monomer": (lambda: lib.final_split_host(None, [], [8, 0], 101), "final_split_host: P = 101, " + PCT),
    "split_kernel_bench R=0": (lambda: lib.split_kernel_bench(SYM, 0), "split_kernel_bench: R = 0, must be an integer, 1 or more"),
    "split_kernel_bench K=True": (lambda: lib.split_kernel_bench(SYM, 2, True), "split_kernel_bench: K = True, must be an integer 1 .. 64"),
    "split_kernel_bench no rows": (lambda: lib.split_kernel_bench(SYM[:0], 2),
                                   "split_kernel_bench: sym must be [n, L] with n >= 1 and 1 <= L <= 512"),
    "split_kernel_bench R=0, no rows": (lambda: lib.split_kernel_bench(SYM[:0], 0), "split_kernel_bench: R = 0, must be an integer, 1 or more"),
    "split_kernel_bench K=65, no rows": (lambda: lib.split_kernel_bench(SYM[:0], 2, 65), "split_kernel_bench: K = 65, must be an integer 1 .. 64"),
    "split_kernel_bench K=0, max_iter=0": (lambda: lib.split_kernel_bench(SYM, 2, 0, 2, 0),
                                           "split_kernel_bench: max_iter = 0, must be an integer, 1 or more"),
    # ---- hor: integers that fit the C types ----
    "hor_rows n_mono=1.5": (lambda: lib.hor_rows([], [], [], [], [], 1.5), "hor_rows: n_mono = 1.5, must be an integer"),
    "hor_rows n_mono=True": (lambda: lib.hor_rows([], [], [], [], [], True), "hor_rows: n_mono = True, must be an integer"),
    "hor_rows n_mono=2^31": (lambda: lib.hor_rows([], [], [], [], [], 1 << 31), "hor_rows: n_mono = 2147483648, must be an integer"),
    "hor_rows G=True": (lambda: lib.hor_rows([], [], [], [], [], 2, True), "hor_rows: G = True, must be an integer"),
    "hor_rows G=2^63": (lambda: lib.hor_rows([], [], [], [], [], 2, BIG), "hor_rows: G = 9223372036854775808, must be an integer"),
    "hor_rows C=2.0": (lambda: lib.hor_rows([], [], [], [], [], 2, 0, 2.0), "hor_rows: C = 2.0, must be an integer"),
    "hor_rows C=True": (lambda: lib.hor_rows([], [], [], [], [], 2, 0, True), "hor_rows: C = True, must be an integer"),
    "hor_rows n_mono=1.5, C=2.0": (lambda: lib.hor_rows([], [], [], [], [], 1.5, 0, 2.0), "hor_rows: n_mono = 1.5, must be an integer"),
    "hor_rows columns differ": (lambda: lib.hor_rows([0, 0], [0, 8], [7, 15], [0, 0], [1], 2), "hor_rows: the five columns differ in length"),
    "hor_rows G=True, columns differ": (lambda: lib.hor_rows([0, 0], [0, 8], [7, 15], [0, 0], [1], 2, True),
                                        "hor_rows: G = True, must be an integer"),
    "final_hor_host n_mono=True": (lambda: lib.final_hor_host(None, True), "final_hor_host: n_mono = True, must be an integer"),
    "final_hor_host G=1.5": (lambda: lib.final_hor_host(None, 2, 1.5), "final_hor_host: G = 1.5, must be an integer"),
    "final_hor_host C=2^63": (lambda: lib.final_hor_host(None, 2, 0, BIG), "final_hor_host: C = 9223372036854775808, must be an integer"),
    "final_hor_host n_mono=True, G=1.5": (lambda: lib.final_hor_host(None, True, 1.5), "final_hor_host: n_mono = True, must be an integer"),
    "final_hor_host G=1.5, C=2^63": (lambda: lib.final_hor_host(None, 2, 1.5, BIG), "final_hor_host: G = 1.5, must be an integer"),
    # ---- the segment calls of --profile and --msa ----
    "profile_segments ends short": (lambda: lib.profile_segments(TEXT, ST, [3], MONOS, [0, 1]),
                                    "profile_segments: starts, ends and pair_tmpl differ in length"),
    "profile_segments pair_tmpl short": (lambda: lib.profile_segments(TEXT, ST, EN, MONOS, [0]),
                                         "profile_segments: starts, ends and pair_tmpl differ in length"),
    "profile_segments ends and pair_tmpl short": (lambda: lib.profile_segments(TEXT, ST, [3], MONOS, [0]),
                                                  "profile_segments: starts, ends and pair_tmpl differ in length"),
    "msa_segments ends short": (lambda: lib.msa_segments(TEXT, ST, [3], MONOS, [0, 1]), "msa_segments: starts, ends and pair_tmpl differ in length"),
    "msa_segments pair_tmpl short": (lambda: lib.msa_segments(TEXT, ST, EN, MONOS, [0]),
                                     "msa_segments: starts, ends and pair_tmpl differ in length"),
    "msa_segments pair_tmpl of no template": (lambda: lib.msa_segments(TEXT, ST, EN, MONOS, [0, 2]),
                                              "msa_segments: pair_tmpl outside the 2 interleaved templates"),
    "msa_segments no template": (lambda: lib.msa_segments(TEXT, ST, EN, [], [0, 1]), "msa_segments: pair_tmpl outside the 0 interleaved templates"),
    "msa_segments ends short, pair_tmpl of no template": (lambda: lib.msa_segments(TEXT, ST, [3], MONOS, [0, 2]),
                                                          "msa_segments: starts, ends and pair_tmpl differ in length"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_refusal(case):
    call, text = CASES[case]
    with pytest.raises(lib.SdError) as e:
        call()
    assert e.value.code == PARAM
    assert e.value.msg == text


def test_autocorr_seed_takes_a_bool_lag():
    """p is the one integer slot of the analyses that takes a bool: True is lag 1"""
    assert lib.autocorr_seed(b"AAAAAAAA", 2, True) == lib.autocorr_seed(b"AAAAAAAA", 2, 1) == (0, 6)


# ---- the command line's checks: one line on stderr and the exit code ----------------------------------------------------------
def ns(**kw):
    base = dict(gpus=None, devices=None, screen=None, records=False, overlap="500", batch_size="5000", lags=None, heatmap=None,
                heatmap_max_pairs=4000000000, ref_compat=False, lenient=False)
    base.update(kw)
    return argparse.Namespace(**base)


def visible():
    n = lib.device_count()
    return "%d HIP device%s visible" % (n, "" if n == 1 else "s")


WORLD = " cannot be combined with a torch.distributed launch (WORLD_SIZE=2)"
SIXTEEN = ",".join(["0"] * 17)
# name -> (check, its arguments, WORLD_SIZE, exit code, the line behind "stringdecomposer: ")
CLI_CASES = {
    "--devices 0,x": (sdmain._device_list, ns(devices="0,x"), 1, 2,
                      lambda: "--devices 0,x: expected a comma-separated list of device ordinals, e.g. 0,2,5"),
    "--devices empty item": (sdmain._device_list, ns(devices="0,"), 1, 2,
                             lambda: "--devices 0,: expected a comma-separated list of device ordinals, e.g. 0,2,5"),
    "--gpus 0": (sdmain._device_list, ns(gpus=0), 1, 2, lambda: "--gpus 0: at least one device"),
    "--gpus 17": (sdmain._device_list, ns(gpus=17), 1, 2, lambda: "--gpus 17: at most 16 device entries in one process"),
    "--devices 17 entries": (sdmain._device_list, ns(devices=SIXTEEN), 1, 2,
                             lambda: "--devices %s: at most 16 device entries in one process" % SIXTEEN),
    "--gpus 2 in a launch": (sdmain._device_list, ns(gpus=2), 2, 2,
                             lambda: "--gpus 2: several devices per process" + WORLD),
    "--devices 0,x in a launch": (sdmain._device_list, ns(devices="0,x"), 2, 2,
                                  lambda: "--devices 0,x: expected a comma-separated list of device ordinals, e.g. 0,2,5"),
    "--gpus 16 of fewer": (sdmain._device_list, ns(gpus=16), 1, 2, lambda: "--gpus 16: 16 devices asked for, " + visible()),
    "--devices 0,999": (sdmain._device_list, ns(devices="0,999"), 1, 2,
                        lambda: "--devices 0,999: device %d does not exist (%s)" % (0 if lib.device_count() == 0 else 999, visible())),
    "--screen in a launch": (sdmain._check_screen, ns(screen=40), 2, 2, lambda: "--screen" + WORLD),
    "--screen -1": (sdmain._check_screen, ns(screen=-1), 1, 2, lambda: "--screen -1: the threshold is an edit distance, at least 0"),
    "--screen --records": (sdmain._check_screen, ns(screen=40, records=True), 1, 2,
                           lambda: "--screen cannot be combined with --records: the record stream holds whole reads"),
    "--screen -v = -b": (sdmain._check_screen, ns(screen=40, overlap="500", batch_size="500"), 1, 2,
                         lambda: "--screen needs -v/--overlap smaller than -b/--batch-size (the regions of a read must not overlap)"),
    "--screen -1 --records": (sdmain._check_screen, ns(screen=-1, records=True), 1, 2,
                              lambda: "--screen -1: the threshold is an edit distance, at least 0"),
    "--lags in a launch": (sdmain._check_lags, ns(lags=4), 2, 2, lambda: "--lags" + WORLD),
    "--lags 0": (sdmain._check_lags, ns(lags=0), 1, 2, lambda: "--lags 0: the number of neighbours is 1 .. 255"),
    "--lags 256": (sdmain._check_lags, ns(lags=256), 1, 2, lambda: "--lags 256: the number of neighbours is 1 .. 255"),
    "--lags --records": (sdmain._check_lags, ns(lags=4, records=True), 1, 2,
                         lambda: "--lags cannot be combined with --records: it is a post-pass over the rows of the final TSV"),
    "--lags 0 --records": (sdmain._check_lags, ns(lags=0, records=True), 1, 2, lambda: "--lags 0: the number of neighbours is 1 .. 255"),
    "--heatmap in a launch": (sdmain._check_heatmap, ns(heatmap="4"), 2, 2, lambda: "--heatmap" + WORLD),
    "--heatmap 0": (sdmain._check_heatmap, ns(heatmap="0"), 1, 2,
                    lambda: "--heatmap 0: expected B or B,W with 1 <= B <= 1048576 rows per bin and W >= 0 (0: no limit) the largest row "
                            "distance of a pair"),
    "--heatmap 4,x": (sdmain._check_heatmap, ns(heatmap="4,x"), 1, 2,
                      lambda: "--heatmap 4,x: expected B or B,W with 1 <= B <= 1048576 rows per bin and W >= 0 (0: no limit) the largest row "
                              "distance of a pair"),
    "--heatmap-max-pairs -1": (sdmain._check_heatmap, ns(heatmap="4", heatmap_max_pairs=-1), 1, 2,
                               lambda: "--heatmap-max-pairs -1: the cap is 0 (no limit) or more"),
    "--heatmap --records": (sdmain._check_heatmap, ns(heatmap="4", records=True), 1, 2,
                            lambda: "--heatmap cannot be combined with --records: it is a post-pass over the rows of the final TSV"),
    "--heatmap 0 --records": (sdmain._check_heatmap, ns(heatmap="0", records=True), 1, 2,
                              lambda: "--heatmap 0: expected B or B,W with 1 <= B <= 1048576 rows per bin and W >= 0 (0: no limit) the "
                                      "largest row distance of a pair"),
    "--lenient --ref-compat": (sdmain._check_lenient, ns(lenient=True, ref_compat=True), 1, PARAM,
                               lambda: "--lenient cannot be combined with --ref-compat, whose purpose is the reference's behaviour (its "
                                       "error for lower case, IUPAC codes and CRLF included): drop one of the two, or convert the input to "
                                       "upper-case ACGTN first"),
    "--lenient in a launch": (sdmain._check_lenient, ns(lenient=True), 2, PARAM,
                              lambda: "--lenient" + WORLD + ": the ranks' convert step reads the files strictly; use --gpus N / --devices "
                                                            "LIST, several GPUs in one process"),
}


@pytest.mark.parametrize("case", list(CLI_CASES))
def test_cli_refusal(case, monkeypatch, capsys):
    check, args, world, code, line = CLI_CASES[case]
    monkeypatch.setenv("WORLD_SIZE", str(world))
    with pytest.raises(SystemExit) as e:
        check(args)
    assert e.value.code == code
    assert capsys.readouterr().err == "stringdecomposer: %s\n" % line()


def test_cli_device_list_without_the_library(monkeypatch, capsys):
    def no_library():
        raise lib.SdError(lib.SD_ERR_INTERNAL, "libsd_hip.so is missing")
    monkeypatch.setattr(lib, "device_count", no_library)
    with pytest.raises(SystemExit) as e:
        sdmain._device_list(ns(gpus=2))
    assert e.value.code == 2
    assert capsys.readouterr().err == "stringdecomposer: --gpus 2: the HIP library is not available (libsd_hip.so is missing)\n"


def test_cli_requests_that_pass(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "1")
    assert sdmain._device_list(ns()) is None and sdmain._device_list(ns(gpus=1)) is None
    for check, args in ((sdmain._check_screen, ns(screen=0)), (sdmain._check_lags, ns(lags=255)),
                        (sdmain._check_heatmap, ns(heatmap="4,0", heatmap_max_pairs=0)), (sdmain._check_lenient, ns(lenient=True))):
        assert check(args) is None
