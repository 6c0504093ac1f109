// The decode attention of a step whose rows may name a chain more than once (speculative decoding: ze_spec.hip): the ROWS
// instantiation of the pipelined per-wave kernel k_attn_decode_wave_long and its launcher, from the kernel's own source -- in a unit of
// its own so that the unit of the plain step compiles to the code it was.
#define ZE_ATTN_ROWS_UNIT
#include "ze_attn_batch.hip"
