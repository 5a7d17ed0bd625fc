// zxc_experiments.h — the ONE gate in front of the experiment switches of the device sources.
//
// The product sources keep only what ships, plus two kinds of switches that leave the decoded / encoded bytes alone:
//   * instruments, to see where the time goes: EXP_TIMES (tools/blocktimes.py), EXP_PHASES and EXP_PIV_PROF (tools/abbench.py)
//     write shader clocks over the status words or the first output bytes of each block; EXP_ENC_CLOCKS (tools/encclk.py) sums
//     the encoder's phase clocks in a device global; ASM_MARKERS (tools/isacount.py) puts comments into the ISA.
//   * plan forcing, to run one decode plan on purpose: EXP_NO_PRE (every coded block to the full kernel), and the runtime
//     ZXC_DEV_DBG_* bits (zxc_dev.h) that zxc_mi355x__set_debug sets in a -DZXC_EXPERIMENT build, and ZXC_EXP_ORDER_SLOTS, which
//     the shim of such a build reads on every launch (tools/ordermix.py: heaviest first, file order, or mixed for a residency).
// Every design that was measured and lost, and every timing-only ablation, has been removed; tools/experiments/SWITCHES.md lists
// them with their results and the commit where they last build. The product Makefile defines none of these names and never
// defines ZXC_EXPERIMENT: a stray -D of one of them in a build without -DZXC_EXPERIMENT stops the compilation here instead of
// producing a silently different library. Included first by every device translation unit.
#ifndef ZXC_EXPERIMENTS_H
#define ZXC_EXPERIMENTS_H
#ifndef ZXC_EXPERIMENT
#if defined(ASM_MARKERS) || defined(EXP_ENC_CLOCKS) || defined(EXP_NO_PRE) || defined(EXP_PHASES) || defined(EXP_PIV_PROF) || defined(EXP_TIMES) || \
    defined(EXP_ORDER_MIX_ROWS) /* (another row count for zxc_dev_order_mix, zxc_dev.h) */ || \
    defined(ZAP_IMAGE_THREADS)  /* (another workgroup size for zxc_append_images_kernel, zxc_append_device.hip) */
#error "an experiment switch is defined without -DZXC_EXPERIMENT: this is not the product configuration (zxc_experiments.h)"
#endif
#endif
#endif
