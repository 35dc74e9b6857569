/* A plain-C99 client of the spectrum regions of include/soundscope_hip.h: a two-stream pass, a list of three regions in one group,
 * the regions' and the group's spectra.  Built and run by tests/test_spectrum_regions_abi.py (CPU: must fail loudly with
 * SS_ERR_DEVICE).  Prints one line of "key=value" pairs. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "soundscope_hip.h"

int main(void)
{
    ss_batch_config cfg;
    ss_batch_layout lay;
    ss_loudness_region list[3];
    ss_batch *b = NULL;
    uint32_t one_first = 0u, one_end = 0u, none_first = 9u, none_end = 9u, all_first = 9u, all_end = 0u;
    uint32_t chunks = 0u, chunk_windows = 0u;
    int rc;
    memset(&cfg, 0, sizeof cfg);
    memset(&lay, 0, sizeof lay);
    cfg.sample_rate = 48000; cfg.channels = 2; cfg.n_streams = 2; cfg.fft_n = 4096; cfg.hop_frames = 1024;
    cfg.flags = SS_BATCH_FFT; cfg.frames_per_stream = 96000;
    list[0].stream = 0u; list[0].first_subblock = 0u; list[0].n_subblocks = 20u; list[0].group = 0u;
    list[1].stream = 1u; list[1].first_subblock = 16u; list[1].n_subblocks = 1u; list[1].group = 0u;
    list[2].stream = 1u; list[2].first_subblock = 0u; list[2].n_subblocks = 1u; list[2].group = SS_REGION_NO_GROUP;
    ss_region_windows(48000u, 4096u, 1024u, 16u, 1u, &one_first, &one_end);
    ss_region_windows(48000u, 4096u, 1024u, 0u, 1u, &none_first, &none_end);
    ss_region_windows(48000u, 4096u, 1024u, 0u, 20u, &all_first, &all_end);
    printf("abi=%d devices=%d sizeof_region=%u one=%u..%u none=%u..%u all=%u..%u ", ss_abi_version(), ss_device_count(), (unsigned)sizeof list[0],
           (unsigned)one_first, (unsigned)one_end, (unsigned)none_first, (unsigned)none_end, (unsigned)all_first, (unsigned)all_end);
    rc = ss_batch_create(&cfg, &b);
    printf("create=%d", rc);
    if (rc == SS_OK) {
        float *mean = NULL, *max = NULL;
        uint32_t counted[6];
        uint64_t pooled[2];
        size_t per = 0, i, finite = 0;
        int early = ss_batch_download_region_spectra(b, 0u, 0u, NULL, NULL, 0u, NULL, 0u);
        int early_plan = ss_batch_spectrum_regions_plan(b, &chunks, &chunk_windows);
        if ((rc = ss_batch_layout_get(b, &lay)) == SS_OK) {
            per = (size_t)lay.fft_channels * lay.n_bins;
            mean = (float *)malloc(3u * per * sizeof *mean);
            max = (float *)malloc(3u * per * sizeof *max);
            if (!mean || !max || lay.fft_channels != 2u) rc = SS_ERR_NOMEM;
        }
        if (rc == SS_OK && (rc = ss_batch_synthesize(b, 7u, 0u)) == SS_OK && (rc = ss_batch_run(b)) == SS_OK &&
            (rc = ss_batch_spectrum_regions(b, list, 3u, 1u)) == SS_OK && (rc = ss_batch_spectrum_regions_plan(b, &chunks, &chunk_windows)) == SS_OK &&
            (rc = ss_batch_download_region_spectra(b, 0u, 3u, mean, max, 3u * per, counted, 6u)) == SS_OK) {
            for (i = 0; i < 2u * per; i++) finite += mean[i] > -400.0f && max[i] > -400.0f;     /* (a NaN fails both) */
            printf(" windows=%u counted=%u,%u,%u finite=%lu of=%lu chunks=%u short=%d beyond=%d", (unsigned)lay.n_windows, (unsigned)counted[0],
                   (unsigned)counted[2], (unsigned)counted[4], (unsigned long)finite, (unsigned long)(2u * per), (unsigned)chunks,
                   ss_batch_download_region_spectra(b, 0u, 3u, mean, NULL, 3u * per - 1u, NULL, 0u),
                   ss_batch_download_region_spectra(b, 2u, 2u, mean, NULL, 3u * per, NULL, 0u));
            if ((rc = ss_batch_download_group_spectra(b, 0u, 1u, mean, max, per, pooled, 2u)) == SS_OK)
                printf(" pooled=%lu", (unsigned long)pooled[0]);
        }
        printf(" early=%d early_plan=%d run=%d", early, early_plan, rc);
        free(mean);
        free(max);
        ss_batch_destroy(b);
    }
    printf("\n");
    return 0;
}
