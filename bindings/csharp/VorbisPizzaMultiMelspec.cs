// P/Invoke binding of include/vorbispizza_multi_melspec.h -- the dispatcher of VorbisPizzaMulti.cs delivering the window batch of
// VorbisPizzaMultiResample.cs (one rate, mono) as (log-)mel spectrogram frames with transforms of 2048, 4096 and 8192 samples, computed
// on the device.  The call is VorbisPizzaMultiLogMel.vpzm_decode_ranges_logmel's, argument for argument: the ranges stay in source
// samples at each stream's own rate; `frames` is the padded row length in OUTPUT samples, every row has 1 + frames / hop feature frames,
// and groupDst[g] is float32 device memory [hi - lo][nMels][T] or [hi - lo][T][nMels] (GpuPcmMelspec.cs names the definition).
// StreamResult.Samples counts the window's output samples; the row of an entry that delivered nothing is the spec's silence row.
// Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class VorbisPizzaMultiMelspec
    {
        private const string Host = "vorbispizza_host";

        [DllImport(Host, CallingConvention = CallingConvention.Cdecl)] public static extern int vpzm_decode_ranges_melspec(VorbisPizzaMulti.DispatcherHandle m, int n, byte** data, ulong* size, VorbisPizzaMultiRanges.Range* ranges, GpuPcmLogMel.LogMelSpec* spec, long frames, void** groupDst, VorbisPizzaMulti.StreamResult* results, VorbisPizzaMulti.Stats* stats);
    }
}
