// P/Invoke binding of include/vorbispizza_multi_featpost.h -- the dispatcher of VorbisPizzaMulti.cs delivering the Kaldi filterbank and
// MFCC window batches of VorbisPizzaMultiFbank.cs and VorbisPizzaMultiMfcc.cs with Kaldi's feature post-processing behind them on the
// device: delta features and mean / variance normalisation over the row or a sliding window (GpuFeatPost.cs names the definition).
// The calls are the existing ones plus a FeatPostSpec: groupDst[g] is float32 device memory [hi - lo][T][DOut] or [hi - lo][DOut][T],
// DOut = D * (DeltaOrder + 1) with D the feature call's columns; the post spec's Layout is the feature spec's.  A row's real frames are
// those of StreamResult.Samples, as for the calls without it; the frames behind them hold the post spec's PadValue, and so does the
// whole row of an entry that delivered nothing.  post == null: the existing call itself.
// Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class VorbisPizzaMultiFeatPost
    {
        private const string Host = "vorbispizza_host";

        [DllImport(Host, CallingConvention = CallingConvention.Cdecl)] public static extern int vpzm_decode_ranges_fbank_post(VorbisPizzaMulti.DispatcherHandle m, int n, byte** data, ulong* size, VorbisPizzaMultiRanges.Range* ranges, GpuPcmFbank.FbankSpec* spec, GpuFeatPost.FeatPostSpec* post, long frames, void** groupDst, VorbisPizzaMulti.StreamResult* results, VorbisPizzaMulti.Stats* stats);
        [DllImport(Host, CallingConvention = CallingConvention.Cdecl)] public static extern int vpzm_decode_ranges_mfcc_post(VorbisPizzaMulti.DispatcherHandle m, int n, byte** data, ulong* size, VorbisPizzaMultiRanges.Range* ranges, GpuPcmMfcc.MfccSpec* spec, GpuFeatPost.FeatPostSpec* post, long frames, void** groupDst, VorbisPizzaMulti.StreamResult* results, VorbisPizzaMulti.Stats* stats);
    }
}
