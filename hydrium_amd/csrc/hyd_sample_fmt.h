/*
 * hyd_sample_fmt.h — the sample formats of the encode entry points, in one place for the C host side and the HIP side.
 *
 * 0, 1, 2 are the drop-in API's HYDSampleFormat (include/libhydrium/libhydrium.h); 3 and 4 (include/hydrium_amd.h) name
 * pixels that already sit in device memory as IEEE binary16 or bfloat16.  Half precision is a STORAGE FORM of the float
 * class: a sample is widened exactly on load and from there on is a float32 sample (hip/hydk_half.h).
 */
#ifndef HYD_SAMPLE_FMT_H_
#define HYD_SAMPLE_FMT_H_

#include <stddef.h>

#define HYD_FMT_UINT8 0
#define HYD_FMT_UINT16 1
#define HYD_FMT_FLOAT32 2
#define HYD_FMT_FLOAT16 3
#define HYD_FMT_BFLOAT16 4

/* what an entry point that reads DEVICE pixels takes */
static inline int hyd_fmt_is_device(int fmt) { return fmt >= HYD_FMT_UINT8 && fmt <= HYD_FMT_BFLOAT16; }
/* what an entry point that reads HOST pixels takes: the reference's three */
static inline int hyd_fmt_is_host(int fmt) { return fmt >= HYD_FMT_UINT8 && fmt <= HYD_FMT_FLOAT32; }
/* float class: 8-byte token records, 72 histogram bins, the non-finite check */
static inline int hyd_fmt_is_float(int fmt) { return fmt >= HYD_FMT_FLOAT32 && fmt <= HYD_FMT_BFLOAT16; }
/* bytes per sample of a format hyd_fmt_is_device accepts (strides are in samples); 0 for anything else */
static inline size_t hyd_fmt_bytes(int fmt) {
    switch (fmt) {
    case HYD_FMT_UINT8:
        return 1;
    case HYD_FMT_UINT16:
    case HYD_FMT_FLOAT16:
    case HYD_FMT_BFLOAT16:
        return 2;
    case HYD_FMT_FLOAT32:
        return 4;
    default:
        return 0;
    }
}

#endif /* HYD_SAMPLE_FMT_H_ */
