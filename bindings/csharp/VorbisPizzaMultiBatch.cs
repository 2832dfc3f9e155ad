// P/Invoke binding of include/vorbispizza_multi_batch.h -- the dispatcher of VorbisPizzaMulti.cs delivering the windows of
// VorbisPizzaMultiRanges.cs as a padded batch in DEVICE memory.  A loader whose model runs on the GPU the decoder ran on asks
// vpzm_batch_partition which entries every group decodes, hands every group its piece of a device tensor
// [n][channels][frames] (or [n][frames][channels]) -- groups on one GPU get consecutive pieces of one array -- and gets entry
// k's window in row k, zeros behind its samples; no PCM crosses the host link.  StreamResult is what vpzm_decode_ranges
// reports; EChannels marks an entry whose stream does not have the batch's channel count.
// Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class VorbisPizzaMultiBatch
    {
        private const string Host = "vorbispizza_host";

        public const int EChannels = -15;             // VPZM_E_CHANNELS: per-entry status, the stream does not have the batch's channel count

        [DllImport(Host, CallingConvention = CallingConvention.Cdecl)] public static extern int vpzm_batch_partition(VorbisPizzaMulti.DispatcherHandle m, int n, int group, int* lo, int* hi);
        [DllImport(Host, CallingConvention = CallingConvention.Cdecl)] public static extern int vpzm_decode_ranges_batch(VorbisPizzaMulti.DispatcherHandle m, int n, byte** data, ulong* size, VorbisPizzaMultiRanges.Range* ranges, int channels, long frames, int outLayout, void** groupDst, VorbisPizzaMulti.StreamResult* results, VorbisPizzaMulti.Stats* stats);
    }
}
