// P/Invoke binding of include/vorbispizza_multi_normalize.h -- the dispatcher of VorbisPizzaMulti.cs delivering the resampled device
// batch of VorbisPizzaMultiResample.cs NORMALISED: every row at zero mean and unit variance over its real samples (wav2vec 2.0's
// feature extractor), at a peak, an RMS level or a programme loudness (measured as VorbisPizzaMultiLoudness.cs measures it, without a
// second decode), or through one gain, with an optional ceiling on the delivered peak.  The arguments up to `stats` are
// vpzm_decode_ranges_resampled's; a NormSpec and an optional array of n NormOut follow.  GpuPcmNormalize.cs is the stage; its header
// states the statistics, their order and the error bound.  Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class VorbisPizzaMultiNormalize
    {
        private const string Host = "vorbispizza_host";

        public const int NormMeanvar = 1, NormPeak = 2, NormRms = 3, NormGain = 4, NormLoudness = 5;  // NormSpec.Mode

        [StructLayout(LayoutKind.Sequential)]
        public struct NormSpec
        {
            public double Target;
            public double Eps;
            public double Ceiling;
            public int Mode;
            public fixed int Reserved[9];
        }

        [StructLayout(LayoutKind.Sequential)]
        public struct NormOut
        {
            public double Gain;
            public double Mean;
            public double Peak;
            public double Loudness;
        }

        [DllImport(Host, CallingConvention = CallingConvention.Cdecl)] public static extern int vpzm_decode_ranges_normalized(VorbisPizzaMulti.DispatcherHandle m, int n, byte** data, ulong* size, VorbisPizzaMultiRanges.Range* ranges, int sampleRate, int channels, int downmix, long frames, int outLayout, void** groupDst, VorbisPizzaMulti.StreamResult* results, VorbisPizzaMulti.Stats* stats, NormSpec* spec, NormOut* records);
    }
}
