// P/Invoke binding of include/vorbispizza_pcm_featpost.h -- Kaldi feature post-processing of a padded batch of float32 feature frames in
// device memory ([rows][T][D] or [rows][D][T]: the tensors of GpuPcmMfcc, GpuPcmFbank and GpuPcmLogMel alike): delta features
// (add-deltas: the scales convolved, the input clamped to a row's REAL frames) and mean / variance normalisation over the row
// (apply-cmvn) or a sliding window (apply-cmvn-sliding), in either order, with the pad frames of every row kept at PadValue.  A host
// fills one FeatRow per row -- which source row, how many real frames, which destination row -- and a FeatPostSpec, asks
// vpz_feat_post_scratch for the float64 elements of scratch memory and makes one vpz_feat_post call, asynchronous on the context's
// stream.  The header states the definition; vpz_feat_delta_scales and vpz_feat_cmn_window give the scales and a frame's window without
// a device.
// Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class GpuFeatPost
    {
        private const string Synth = "vorbispizza_synth";

        public const int NormNone = 0, NormRow = 1, NormSliding = 2;       // FeatPostSpec.Norm
        public const int PostNormFirst = 0, PostDeltasFirst = 1;           // FeatPostSpec.Order
        public const int FeatColumnsFirst = 0, FeatFramesFirst = 1;        // FeatPostSpec.Layout: [rows][D][T] or [rows][T][D]
        public const int FeatMaxColumns = 256;                             // VPZ_FEAT_MAX_COLUMNS
        public const int FeatMaxDeltaOrder = 3;                            // VPZ_FEAT_MAX_DELTA_ORDER
        public const int FeatMaxDeltaWindow = 8;                           // VPZ_FEAT_MAX_DELTA_WINDOW
        public const int FeatMaxCmnWindow = 1 << 20;                       // VPZ_FEAT_MAX_CMN_WINDOW
        public const int FeatChunk = 64;                                   // VPZ_FEAT_CHUNK

        [StructLayout(LayoutKind.Sequential)]
        public struct FeatRow
        {
            public long SrcRow;
            public long RealFrames;
            public long Row;
        }

        [StructLayout(LayoutKind.Sequential)]
        public struct FeatPostSpec
        {
            public double VarFloor;
            public double PadValue;
            public int Norm;
            public int NormVars;
            public int Center;
            public int CmnWindow;
            public int MinWindow;
            public int DeltaOrder;
            public int DeltaWindow;
            public int Order;
            public int Layout;
            public fixed int Reserved[11];
        }

        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_feat_delta_scales(FeatPostSpec* spec, int i, float* scales, long capacity);
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_feat_cmn_window(FeatPostSpec* spec, long t, long n, long* a, long* b);
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_feat_post_scratch(FeatPostSpec* spec, int nRows, long T, int D, long* elems);
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_feat_post(IntPtr ctx, void* srcDev, long srcRows, long T, int D, FeatPostSpec* spec, int nRows, FeatRow* rows, void* dstDev, long dstRows, void* scratchDev, long scratchElems);
    }
}
