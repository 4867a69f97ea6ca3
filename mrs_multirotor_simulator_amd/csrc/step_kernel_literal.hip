// LITERAL flavour of the fused step kernel: reference operation order, compiled with -ffp-contract=off.
#define MRS_FAST 0
#include "step_device.inc"
#include "rollout_device.inc"
#include "rollout_rate_device.inc"
#include "rollout_cost_device.inc"
#include "rollout_tick_device.inc"
