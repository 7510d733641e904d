"""Command line of backend/main.py (reference backend/tools/args_handler.py:6-30): same flags,
same defaults, --inpaint-mode parsed into the InpaintMode enum.  All five modes run on the MI355X (opencv: inpaint/opencv_inpaint.py)."""
import argparse

from .constant import InpaintMode


def build_parser():
    parser = argparse.ArgumentParser(description="Video Subtitle Remover Command Line Tool")
    parser.add_argument("--input", "-i", required=True, type=str, help="Input video file path")
    parser.add_argument("--output", "-o", required=False, type=str, default=None,
                        help="Output video file path (optional)")
    parser.add_argument("--subtitle-area-coords", "-c", action="append", nargs=4, type=int,
                        metavar=("YMIN", "YMAX", "XMIN", "XMAX"),
                        help="Subtitle area coordinates (ymin ymax xmin xmax). Can be specified multiple times "
                             "for multiple areas.")
    parser.add_argument("--inpaint-mode", type=str, default="sttn-auto",
                        choices=[mode.name.lower().replace("_", "-") for mode in InpaintMode],
                        help="Inpaint mode, default is sttn-auto")
    # not in the reference: what a *.y4m sink holds (overrides VSR_Y4M_OUT)
    parser.add_argument("--y4m-out", type=str, default=None, choices=["444", "source"],
                        help="*.y4m output: 444 = 8-bit 4:4:4 (default), source = the format of the *.y4m input, untouched samples kept")
    # not in the reference: a clip over VSR_RESIDENT_GB stays on the GPU as a sequence of resident windows (sets VSR_IO_RESIDENT=windows)
    parser.add_argument("--resident-windows", action="store_true",
                        help="a *.y4m clip too large for VSR_RESIDENT_GB runs as HBM-resident windows instead of the host-frame loop")
    # not in the reference: sttn-auto chunks / sttn-det intervals restart at scene cuts and look back at the source frames in front of them
    parser.add_argument("--scene-split", action="store_true",
                        help="sttn-auto, sttn-det: no chunk / batch straddles a scene cut (one scene-detection pass over the video first); "
                             "sets VSR_SCENE_SPLIT=1")
    parser.add_argument("--sttn-context", type=int, default=None, metavar="N",
                        help="sttn-auto, sttn-det: every chunk / batch also sees the N source frames in front of it (0 <= N <= the chunk "
                             "length / the batch limit; never across a scene cut with --scene-split, sttn-det: never in front of its "
                             "subtitle interval); sets VSR_STTN_CONTEXT")
    parser.add_argument("--sttn-lookahead", type=int, default=None, metavar="M",
                        help="sttn-auto, sttn-det: every chunk / batch also sees the M source frames behind it (0 <= M <= the chunk "
                             "length / the batch limit; never across a scene cut with --scene-split, sttn-det: never behind its "
                             "subtitle interval); combines with --sttn-context; sets VSR_STTN_LOOKAHEAD")
    # not in the reference: every mode ends its plugin call with a mask-exact, feathered composite (tools/seam_feather.py)
    parser.add_argument("--seam-feather", type=int, default=None, metavar="F",
                        help="every mode: outside the pixels a plugin blends under, the written frame is the source bit for bit; inside, "
                             "the fill ramps in over F pixels (1 = hard composite, 0 = off, at most 64); one process; sets VSR_SEAM_FEATHER")
    # not in the reference: every mode puts the source's grain back inside the pixels it inpainted (tools/regrain.py)
    parser.add_argument("--regrain", type=int, default=None, metavar="P",
                        help="every mode: measure the source's noise in a ring around the inpainted pixels and add P percent of what the "
                             "fill lacks back inside them (100 = match the source, 0 = off, at most 200); one process; sets VSR_REGRAIN")
    # not in the reference: every mode steadies its fill over time inside the pixels it inpainted (tools/deflicker.py)
    parser.add_argument("--deflicker", type=int, default=None, metavar="R",
                        help="every mode: inside the inpainted pixels, mix every frame's fill with the fills of the R frames before and "
                             "after it in the same batch, as far as the picture around them stood still (0 = off, at most 8); one process; "
                             "sets VSR_DEFLICKER")
    # not in the reference: every mode levels its fill's tone to the picture across the seam of the pixels it inpainted (tools/tone_match.py)
    parser.add_argument("--tone-match", type=int, default=None, metavar="S",
                        help="every mode: measure the step between the picture just outside the inpainted pixels and the fill just inside "
                             "them and add S percent of it, faded smoothly into the interior, to the fill (100 = level the seam, 0 = off); "
                             "one process; sets VSR_TONE_MATCH")
    # not in the reference: every mode keeps the source wherever its fill only repeats it (tools/glyph_key.py)
    parser.add_argument("--glyph-key", type=int, default=None, metavar="T",
                        help="every mode: inside the inpainted pixels, keep the source bit for bit wherever the fill differs from it by "
                             "less than T levels in the 3x3 mean, and put the fill in only around the pixels where it differs by more, "
                             "grown by 4 pixels and ramped back over 4 more (0 = off, at most 128); one process; sets VSR_GLYPH_KEY")
    parser.add_argument("--glyph-hold", type=int, default=None, metavar="K",
                        help="with --glyph-key T: a pixel that differs by at least (T + 1) // 2 levels stays filled while one of the K "
                             "frames before or after it in the same batch differs by T or more within one pixel of it, so that a glyph "
                             "that hovers about T does not flicker (0 = off, at most 8); sets VSR_GLYPH_HOLD")
    # not in the reference: every mode fills from the real picture of neighbouring frames where it can (tools/borrow.py)
    parser.add_argument("--borrow", type=int, default=None, metavar="B",
                        help="with --glyph-key T: where the key would show fill and one of the B frames before or after in the same batch "
                             "shows the real picture at that pixel, take that frame's pixel instead of the fill, if the picture around the "
                             "inpainted pixels stood still between the two and the pixel lies within 24 levels of the fill (0 = off, at "
                             "most 8); sets VSR_BORROW")
    parser.add_argument("--borrow-pan", type=int, default=None, metavar="P",
                        help="with --borrow B: follow a camera that pans by whole pixels: per pair of frames a shift of up to P pixels "
                             "per frame step, found on the picture around the inpainted pixels, is used where the picture did not stand "
                             "still, and the other frame's pixel is read at the shifted place (0 = off, at most 8); sets VSR_BORROW_PAN")
    # not in the reference: every mode finds the static overlays of the clip itself and inpaints them on every frame (tools/logo_scan.py)
    parser.add_argument("--logo-scan", action="store_true",
                        help="every mode: one pass over the clip on the GPU first finds the rectangles that hold a static overlay (a "
                             "station logo, a channel bug, a burnt-in watermark: edges that stay put while the picture around them moves) "
                             "and inpaints them on every frame; sttn-auto: they join the -c boxes and, without -c, replace the "
                             "whole-frame default; the other modes: -c keeps restricting the text detector only; finds nothing in a "
                             "static shot and no overlay larger than a third of the frame; needs 16 frames; one process; sets VSR_LOGO_SCAN=1")
    # not in the reference: a translucent overlay found by --logo-scan is un-mixed, not inpainted (tools/unblend.py)
    parser.add_argument("--logo-unblend", action="store_true",
                        help="with --logo-scan: an overlay that is translucent, I = (1 - a) B + a L, gives the real picture back by a "
                             "division instead of an inpainted one: per pixel of a found area the gain 1 - a and the offset a L are "
                             "estimated from the frames the scan sampled, and every frame's area gets (I - a L) / (1 - a) of its "
                             "source; the fill stays under the opaque part, and an area whose overlay is opaque, too faint, in a "
                             "still shot or crossed by a text box is inpainted as before; sets VSR_LOGO_UNBLEND=1")
    # not in the reference: opencv mode's fill itself (inpaint/opencv_inpaint.py)
    parser.add_argument("--opencv-fill", type=str, default=None, metavar="{telea,exemplar}",
                        help="--inpaint-mode opencv: telea = OpenCV's Telea fill (default), exemplar = a PatchMatch exemplar fill, coarse to "
                             "fine, that copies real texture from the picture around the hole instead of diffusing the rim inwards; needs "
                             "no weights; sets VSR_OPENCV_FILL")
    # not in the reference: which text detector the detector-driven modes use (tools/stroke_det.py)
    parser.add_argument("--text-detect", type=str, default=None, metavar="{model,strokes}",
                        help="the text detector of sttn-det, lama, propainter, opencv and picture mode: model = the PP-OCRv5 network "
                             "(default; needs VSR_DET_MODEL_DIR and its weights), strokes = a weight-free detector on the GPU of "
                             "stroke-like text (thin bright or dark strokes with strong contrast, both ways, dense along a line: a "
                             "burnt-in subtitle with an outline or a shadow); it misses text without contrast, strokes wider than 6 "
                             "analysis pixels, a single very short word and vertical text, and takes dense fine texture for text; one "
                             "process; sets VSR_TEXT_DETECT")
    return parser


def parse_args(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.opencv_fill is not None:
        from ..inpaint.opencv_inpaint import fill_option

        try:
            args.opencv_fill = fill_option(args.opencv_fill)
        except ValueError as e:
            parser.error(f"--opencv-fill: {e}")
        if args.opencv_fill == "exemplar" and args.inpaint_mode != "opencv":
            parser.error("--opencv-fill exemplar: it is the fill of --inpaint-mode opencv, and the mode is " + args.inpaint_mode)
    if args.text_detect is not None:
        from .stroke_det import detect_option

        try:
            args.text_detect = detect_option(args.text_detect)
        except ValueError as e:
            parser.error(f"--text-detect: {e}")               # (strokes with sttn-auto is refused by the run, which knows a picture from a video)
    if args.seam_feather is not None:
        from .seam_feather import feather_option

        try:
            feather_option(args.seam_feather)
        except ValueError as e:
            parser.error(f"--seam-feather: {e}")
    if args.regrain is not None:
        from .regrain import regrain_option

        try:
            regrain_option(args.regrain)
        except ValueError as e:
            parser.error(f"--regrain: {e}")
    if args.deflicker is not None:
        from .deflicker import deflicker_option

        try:
            deflicker_option(args.deflicker)
        except ValueError as e:
            parser.error(f"--deflicker: {e}")
    if args.tone_match is not None:
        from .tone_match import tone_option

        try:
            tone_option(args.tone_match)
        except ValueError as e:
            parser.error(f"--tone-match: {e}")
    if args.glyph_key is not None:
        from .glyph_key import key_option

        try:
            key_option(args.glyph_key)
        except ValueError as e:
            parser.error(f"--glyph-key: {e}")
    if args.glyph_hold is not None:
        from .glyph_key import hold_option, key_option

        try:
            if hold_option(args.glyph_hold) and not key_option(args.glyph_key):
                raise ValueError("it holds the seeds of --glyph-key T, which is off: give both")
        except ValueError as e:
            parser.error(f"--glyph-hold: {e}")
    if args.borrow is not None:
        from .borrow import borrow_option
        from .glyph_key import key_option

        try:
            if borrow_option(args.borrow) and not key_option(args.glyph_key):
                raise ValueError("it borrows where --glyph-key T would show fill, and that is off: give both")
        except ValueError as e:
            parser.error(f"--borrow: {e}")
    if args.borrow_pan is not None:
        from .borrow import borrow_option, pan_option

        try:
            if pan_option(args.borrow_pan) and not borrow_option(args.borrow):
                raise ValueError("it says how far --borrow B follows a pan, and that is off: give both")
        except ValueError as e:
            parser.error(f"--borrow-pan: {e}")
    if args.logo_unblend and not args.logo_scan:
        parser.error("--logo-unblend: it un-mixes the areas --logo-scan finds, and that is off: give both")
    args.inpaint_mode = InpaintMode[args.inpaint_mode.replace("-", "_").upper()]
    if args.subtitle_area_coords is None:
        args.subtitle_area_coords = []
    return args
