/* zxc_dev_order_mix (zxc_amd/csrc/zxc_dev.h) as the host compiles it, for tests/test_order_mix_cpu.py. Test infrastructure. */
#include <stdint.h>

#include "../../zxc_amd/csrc/zxc_dev.h"

uint32_t t_order_mix_rows(void) { return ZXC_DEV_ORDER_MIX_ROWS; }
/* out[pos] = index in order[] of sorted position pos, for every pos of a launch of n blocks */
void t_order_mix_all(uint32_t n, uint32_t slots, uint32_t* out) {
    for (uint32_t pos = 0; pos < n; pos++) out[pos] = zxc_dev_order_mix(pos, n, slots);
}
