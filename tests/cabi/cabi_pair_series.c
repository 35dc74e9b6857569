/* A plain-C99 client of the pair series and pair regions of include/soundscope_hip.h: the series of what was synthesised (no pass)
 * for the default pair and for (1, 0) + (0, 0), then every stream as a region of one group and one second of stream 0 outside every
 * group.  Built and run by tests/test_pair_series_abi.py (CPU: must fail loudly with SS_ERR_DEVICE).  Prints one line of
 * "key=value" pairs. */
#include <stdio.h>
#include <string.h>

#include "soundscope_hip.h"

int main(void)
{
    ss_batch_config cfg;
    ss_batch *b = NULL;
    ss_loudness_region reg[5];
    ss_pair_region_config rc_cfg;
    ss_channel_pair pairs[2];
    static ss_pair_entry series[50 * 2];
    static ss_region_pair res[5 * 2];
    static ss_group_pair grp[1 * 2];
    uint32_t s, tile = 0u, cap = 0u, n_pairs = 0u, n_entries = 0u;
    int rc;
    memset(&cfg, 0, sizeof cfg);
    cfg.sample_rate = 48000; cfg.channels = 2; cfg.n_streams = 4; cfg.fft_n = 4096; cfg.hop_frames = 1024;
    cfg.flags = SS_BATCH_TRUE_PEAK; cfg.frames_per_stream = 48000 * 5 - 100;
    for (s = 0; s < 4u; s++) { reg[s].stream = s; reg[s].first_subblock = 0u; reg[s].n_subblocks = 50u; reg[s].group = 0u; }
    reg[4].stream = 0u; reg[4].first_subblock = 10u; reg[4].n_subblocks = 10u; reg[4].group = SS_REGION_NO_GROUP;
    rc_cfg.threshold = 0.0; rc_cfg.power_floor = 0.0; rc_cfg.min_run = 1u; rc_cfg.reserved = 0u;
    pairs[0].a = 1u; pairs[0].b = 0u; pairs[1].a = 0u; pairs[1].b = 0u;
    printf("abi=%d devices=%d sizeof_pair=%u sizeof_entry=%u sizeof_config=%u sizeof_region_pair=%u sizeof_group_pair=%u ", ss_abi_version(),
           ss_device_count(), (unsigned)sizeof pairs[0], (unsigned)sizeof series[0], (unsigned)sizeof rc_cfg, (unsigned)sizeof res[0],
           (unsigned)sizeof grp[0]);
    rc = ss_batch_create(&cfg, &b);
    printf("create=%d", rc);
    if (rc == SS_OK) {
        if ((rc = ss_batch_synthesize(b, 7u, 0u)) == SS_OK && (rc = ss_batch_pair_series(b, NULL, 0u)) == SS_OK &&
            (rc = ss_batch_download_pair_series(b, 0u, series, 50u, &n_entries)) == SS_OK) {
            if ((rc = ss_batch_pair_series(b, pairs, 2u)) == SS_OK && (rc = ss_batch_pair_series_plan(b, &tile, &cap, &n_pairs)) == SS_OK &&
                (rc = ss_batch_download_pair_series(b, 0u, series, 50u, &n_entries)) == SS_OK &&
                (rc = ss_batch_pair_regions(b, reg, 5u, 1u, &rc_cfg)) == SS_OK && (rc = ss_batch_download_region_pairs(b, res, 10u)) == SS_OK &&
                (rc = ss_batch_download_group_pairs(b, grp, 2u)) == SS_OK)
                printf(" tile=%u cap=%u pairs=%u entries=%u tail_frames=%u same_power=%d item_frames=%lu album_frames=%lu album_active=%lu",
                       (unsigned)tile, (unsigned)cap, (unsigned)n_pairs, (unsigned)n_entries, (unsigned)series[49 * 2].frames,
                       series[49 * 2 + 1].s_ab == series[49 * 2].s_bb, (unsigned long)res[4 * 2].frames,
                       (unsigned long)grp[0].frames, (unsigned long)grp[1].n_active);
        }
        printf(" run=%d", rc);
        ss_batch_destroy(b);
    }
    printf("\n");
    return 0;
}
