/* A plain-C99 client of the loudness regions of include/soundscope_hip.h: one pass, then every stream as a region of one album
 * group and a three-second range of stream 0 outside every group.  Built and run by tests/test_loudness_regions_abi.py (CPU: must
 * fail loudly with SS_ERR_DEVICE).  Prints one line of "key=value" pairs. */
#include <stdio.h>
#include <string.h>

#include "soundscope_hip.h"

int main(void)
{
    ss_batch_config cfg;
    ss_batch *b = NULL;
    ss_loudness_region reg[5];
    ss_region_result res[5];
    ss_group_result grp[1];
    static uint64_t hist[2000];
    uint32_t s;
    int rc;
    memset(&cfg, 0, sizeof cfg);
    cfg.sample_rate = 48000; cfg.channels = 2; cfg.n_streams = 4; cfg.fft_n = 4096; cfg.hop_frames = 1024;
    cfg.flags = SS_BATCH_LUFS; cfg.frames_per_stream = 48000 * 5;
    for (s = 0; s < 4u; s++) { reg[s].stream = s; reg[s].first_subblock = 0u; reg[s].n_subblocks = 50u; reg[s].group = 0u; }
    reg[4].stream = 0u; reg[4].first_subblock = 10u; reg[4].n_subblocks = 30u; reg[4].group = SS_REGION_NO_GROUP;
    printf("abi=%d devices=%d sizeof_region=%u sizeof_result=%u sizeof_group=%u no_group=%u ", ss_abi_version(), ss_device_count(),
           (unsigned)sizeof reg[0], (unsigned)sizeof res[0], (unsigned)sizeof grp[0], (unsigned)SS_REGION_NO_GROUP);
    rc = ss_batch_create(&cfg, &b);
    printf("create=%d", rc);
    if (rc == SS_OK) {
        if ((rc = ss_batch_synthesize(b, 7u, 0u)) == SS_OK && (rc = ss_batch_run(b)) == SS_OK &&
            (rc = ss_batch_loudness_regions(b, reg, 5u, 1u)) == SS_OK && (rc = ss_batch_download_region_results(b, res, 5u)) == SS_OK &&
            (rc = ss_batch_download_group_results(b, grp, 1u)) == SS_OK && (rc = ss_batch_group_histograms(b, 0u, hist)) == SS_OK)
            printf(" album=%.6f album_blocks=%u item=%.6f item_blocks=%u item_st=%u item_at=%u", grp[0].integrated_lufs,
                   (unsigned)grp[0].n_gating_blocks, res[4].integrated_lufs, (unsigned)res[4].n_gating_blocks,
                   (unsigned)res[4].n_st_blocks, (unsigned)res[4].max_shortterm_at);
        printf(" run=%d", rc);
        ss_batch_destroy(b);
    }
    printf("\n");
    return 0;
}
