/* A plain-C99 client of the peak series and peak regions of include/soundscope_hip.h: the series of what was synthesised (no pass),
 * then every stream as a region of one group and one second of stream 0 outside every group, against a ceiling of -1 dBTP.  Built
 * and run by tests/test_peak_series_abi.py (CPU: must fail loudly with SS_ERR_DEVICE).  Prints one line of "key=value" pairs. */
#include <stdio.h>
#include <string.h>

#include "soundscope_hip.h"

int main(void)
{
    ss_batch_config cfg;
    ss_batch *b = NULL;
    ss_loudness_region reg[5];
    ss_region_peaks res[5];
    ss_group_peaks grp[1];
    static ss_peak_entry series[50 * 2];
    static float ch_true[5 * 2], ch_sample[5 * 2];
    uint32_t s, tile = 0u, cap = 0u, n_entries = 0u;
    int rc;
    memset(&cfg, 0, sizeof cfg);
    cfg.sample_rate = 48000; cfg.channels = 2; cfg.n_streams = 4; cfg.fft_n = 4096; cfg.hop_frames = 1024;
    cfg.flags = SS_BATCH_TRUE_PEAK; cfg.frames_per_stream = 48000 * 5 - 100;
    for (s = 0; s < 4u; s++) { reg[s].stream = s; reg[s].first_subblock = 0u; reg[s].n_subblocks = 50u; reg[s].group = 0u; }
    reg[4].stream = 0u; reg[4].first_subblock = 10u; reg[4].n_subblocks = 10u; reg[4].group = SS_REGION_NO_GROUP;
    printf("abi=%d devices=%d sizeof_entry=%u sizeof_region_peaks=%u sizeof_group_peaks=%u ", ss_abi_version(), ss_device_count(),
           (unsigned)sizeof series[0], (unsigned)sizeof res[0], (unsigned)sizeof grp[0]);
    rc = ss_batch_create(&cfg, &b);
    printf("create=%d", rc);
    if (rc == SS_OK) {
        if ((rc = ss_batch_synthesize(b, 7u, 0u)) == SS_OK && (rc = ss_batch_peak_series_plan(b, &tile, &cap)) == SS_OK &&
            (rc = ss_batch_peak_series(b)) == SS_OK && (rc = ss_batch_download_peak_series(b, 0u, series, 50u, &n_entries)) == SS_OK &&
            (rc = ss_batch_peak_regions(b, reg, 5u, 1u, 0.891)) == SS_OK && (rc = ss_batch_download_region_peaks(b, res, 5u)) == SS_OK &&
            (rc = ss_batch_download_group_peaks(b, grp, 1u)) == SS_OK &&
            (rc = ss_batch_download_region_channel_peaks(b, ch_true, ch_sample, 10u)) == SS_OK)
            printf(" tile=%u cap=%u entries=%u tail_frame=%u album_tp=%.6f album_region=%u item_tp=%.6f item_frame=%lu item_overs=%u item_ch0=%.6f",
                   (unsigned)tile, (unsigned)cap, (unsigned)n_entries, (unsigned)series[49 * 2].sample_peak_frame, grp[0].true_peak,
                   (unsigned)grp[0].true_peak_region, res[4].true_peak, (unsigned long)res[4].true_peak_frame, (unsigned)res[4].n_over,
                   (double)ch_true[4 * 2]);
        printf(" run=%d", rc);
        ss_batch_destroy(b);
    }
    printf("\n");
    return 0;
}
