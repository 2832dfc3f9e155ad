// P/Invoke binding of include/vorbispizza_multi_loudness.h -- the dispatcher of VorbisPizzaMulti.cs measuring windows of streams, or
// whole streams (ranges null), for programme loudness on the device: the batch call of VorbisPizzaMultiBatch.cs with
// GpuPcmLoudness.vpz_pcm_loudness as its delivery, at every stream's own rate and channel count.  No PCM comes down: outRecords[k] is
// entry k's integrated loudness (LUFS, negative infinity with fewer than four 100 ms steps or nothing kept by the gate), its sample
// peak, its whole steps and the 400 ms blocks behind the value.  StreamResult.Samples counts the samples measured; an entry that
// delivered nothing, whatever its status, has { -infinity, 0, 0, 0 }.
// Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class VorbisPizzaMultiLoudness
    {
        private const string Host = "vorbispizza_host";

        [StructLayout(LayoutKind.Sequential)]
        public struct Loudness
        {
            public double Integrated;
            public double Peak;
            public long Steps;
            public long BlocksKept;
        }

        [DllImport(Host, CallingConvention = CallingConvention.Cdecl)] public static extern int vpzm_measure_loudness(VorbisPizzaMulti.DispatcherHandle m, int n, byte** data, ulong* size, VorbisPizzaMultiRanges.Range* ranges, Loudness* outRecords, VorbisPizzaMulti.StreamResult* results, VorbisPizzaMulti.Stats* stats);
    }
}
