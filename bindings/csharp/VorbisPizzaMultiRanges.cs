// P/Invoke binding of include/vorbispizza_multi_ranges.h -- the dispatcher of VorbisPizzaMulti.cs decoding a WINDOW of samples
// out of every stream in one batched call.  A host creates its dispatcher as before (VorbisPizzaMulti.vpzm_create), fills one
// Range per container -- the same container may appear many times -- and gets, per entry, only the packets its window needs
// decoded: the pre-roll packet before the window's first sample through the packet of its last.  A window of a clean stream
// is bit for bit the same samples of the whole decode; StreamResult.Samples says how many arrived, .Packets how many packets
// were decoded for them.  Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class VorbisPizzaMultiRanges
    {
        private const string Host = "vorbispizza_host";

        public const int ERange = -14;                // VPZM_E_RANGE: per-stream status, start < 0 or beyond the stream's total samples

        [StructLayout(LayoutKind.Sequential)]
        public struct Range                           // vpzm_range: samples per channel
        {
            public long Start;
            public long Count;                        // < 0: to the end of the stream
        }

        [DllImport(Host, CallingConvention = CallingConvention.Cdecl)] public static extern int vpzm_decode_ranges(VorbisPizzaMulti.DispatcherHandle m, int n, byte** data, ulong* size, Range* ranges, int outLayout, void* pcmOut, long* pcmOffset, long* pcmCapacity, VorbisPizzaMulti.StreamResult* results, VorbisPizzaMulti.Stats* stats);
    }
}
