// P/Invoke binding of include/vorbispizza_pcm_r128.h -- what an EBU R 128 scanner needs beside the integrated loudness of
// GpuPcmLoudness.cs: the true peak of windows of an interleaved float32 device PCM array, on the device, and the loudness range and the
// maximum momentary and short-term loudness of their step sums, on the host.  A host fills one GpuPcmPack.PackRow per window, as for
// vpz_pcm_loudness, and makes one vpz_pcm_true_peak call per sample rate: truePeakDev[r] (float) gets the largest magnitude of the window
// oversampled 4 times below 96 000 Hz, twice below 192 000 Hz and not at all from there on (a Hann-windowed sinc of 12 taps per phase),
// samplePeakDev[r] (float, may be null) its sample peak, asynchronously on the context's stream.  vpz_loudness_range (EBU Tech 3342) and
// vpz_loudness_maxima take a row's first samples / S step sums of vpz_pcm_loudness.  The header states the definitions;
// vpz_true_peak_filter gives the factor and the interpolator of a rate without a device.
// Out of scope: a gain on delivery, int16 sources, per-channel peaks, another oversampling.
// Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class GpuPcmR128
    {
        private const string Synth = "vorbispizza_synth";

        public const int TruePeakTaps = 12;        // VPZ_TRUE_PEAK_TAPS
        public const int TruePeakMaxCoeffs = 49;   // VPZ_TRUE_PEAK_MAX_COEFFS

        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_true_peak_filter(int sampleRate, int* factor, double* h);
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_pcm_true_peak(IntPtr ctx, void* srcDev, long srcElems, int channels, int sampleRate, int nRows, GpuPcmPack.PackRow* rows, float* truePeakDev, float* samplePeakDev, long dstRows);
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_loudness_range(double* sums, long nSteps, int stepLen, double* range, double* low, double* high, long* blocksKept);
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_loudness_maxima(double* sums, long nSteps, int stepLen, double* momentaryMax, double* shortTermMax);
    }
}
