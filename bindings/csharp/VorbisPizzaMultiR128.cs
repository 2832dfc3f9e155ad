// P/Invoke binding of include/vorbispizza_multi_r128.h -- the dispatcher of VorbisPizzaMulti.cs measuring windows of streams, or whole
// streams (ranges null), for everything an EBU R 128 scanner reports: VorbisPizzaMultiLoudness.vpzm_measure_loudness -- the same
// arguments, statuses, partition, routes and fall-backs -- with GpuPcmR128.vpz_pcm_true_peak as one more launch of its delivery and the
// loudness range and the maxima beside the gate.  No PCM comes down: outRecords[k] is entry k's integrated loudness, its loudness range
// with the two percentile levels, its maximum momentary and short-term loudness, its true peak and its sample peak, its whole steps and
// the blocks behind the integrated value and the range.  Integrated, SamplePeak, Steps and BlocksKept are vpzm_measure_loudness's bits.
// An entry that delivered nothing, whatever its status, has { -infinity, 0, -infinity, -infinity, -infinity, -infinity, 0, 0, 0, 0, 0 }.
// Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class VorbisPizzaMultiR128
    {
        private const string Host = "vorbispizza_host";

        [StructLayout(LayoutKind.Sequential)]
        public struct R128
        {
            public double Integrated;
            public double Range;
            public double RangeLow;
            public double RangeHigh;
            public double MomentaryMax;
            public double ShortTermMax;
            public double TruePeak;
            public double SamplePeak;
            public long Steps;
            public long BlocksKept;
            public long RangeBlocks;
        }

        [DllImport(Host, CallingConvention = CallingConvention.Cdecl)] public static extern int vpzm_measure_r128(VorbisPizzaMulti.DispatcherHandle m, int n, byte** data, ulong* size, VorbisPizzaMultiRanges.Range* ranges, R128* outRecords, VorbisPizzaMulti.StreamResult* results, VorbisPizzaMulti.Stats* stats);
    }
}
