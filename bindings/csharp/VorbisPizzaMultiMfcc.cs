// P/Invoke binding of include/vorbispizza_multi_mfcc.h -- the dispatcher of VorbisPizzaMulti.cs delivering the window batch of
// VorbisPizzaMultiResample.cs (one rate, mono) as Kaldi MFCC feature frames computed on the device.  The ranges stay in source samples
// at each stream's own rate; `frames` is the padded row length in OUTPUT samples, every row has 1 + (frames - win) / hop feature frames,
// and groupDst[g] is float32 device memory [hi - lo][T][nCeps] or [hi - lo][nCeps][T] (GpuPcmMfcc.cs names the definition).
// StreamResult.Samples counts the window's output samples J: the row's first 1 + (J - win) / hop frames are real (none below win), the
// others hold the spec's PadValue, and so does the whole row of an entry that delivered nothing.
// Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class VorbisPizzaMultiMfcc
    {
        private const string Host = "vorbispizza_host";

        [DllImport(Host, CallingConvention = CallingConvention.Cdecl)] public static extern int vpzm_decode_ranges_mfcc(VorbisPizzaMulti.DispatcherHandle m, int n, byte** data, ulong* size, VorbisPizzaMultiRanges.Range* ranges, GpuPcmMfcc.MfccSpec* spec, long frames, void** groupDst, VorbisPizzaMulti.StreamResult* results, VorbisPizzaMulti.Stats* stats);
    }
}
