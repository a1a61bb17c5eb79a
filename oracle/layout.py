"""The one table of state-matrix rows and metric slots the task oracles index by (include/wheeledlab_amd.h: WlStateField,
WlMetric).  Plain numbers, no import of the product: tests/test_abi_cpu.py holds every name here to wheeledlab_amd._abi."""

# WlStateField: pose, velocities (world frame), wheel spin bl br fl fr, steering joint -- the rows before ACT0 are the ones a step
# integrates and checks for non-finite values
PX, QW, VX, WX, WHEEL, STEER_POS, STEER_VEL, ACT0 = 0, 3, 7, 10, 13, 17, 18, 19
TIMER_HF, TIMER_LF, MU_S, MU_D, DAMP, MASS, EPSUM0 = 21, 22, 23, 24, 25, 26, 27
DRIFT_ROWS = 35          # EPSUM0 + 8: the drift oracle's matrix ends with the episode sums ...
CMD_BX, CMD_BY, TGT_X, TGT_Y, TGT_H, CMD_TIMER = 35, 36, 37, 38, 39, 40   # ... the elevation command manager's rows follow
S_COUNT = 41

# WlMetric
M_EPSUM0, M_RESETS, M_TIMEOUTS, M_TERM0, M_NONFINITE, M_EPLEN, M_COUNT = 0, 8, 9, 10, 14, 15, 16
