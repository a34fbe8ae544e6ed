"""The project's own 8 x 8 bitmap font, as data: one 64-bit word per glyph, bit 8 * row + col = cell (col, row), row 0 on top,
column 0 on the left -- the layout a GLYPH record of pp_draw_overlay_u8 carries (include/pyrapose_hip.h), so the kernel holds no
font.  Drawn for this project on a 5 x 7 grid (rows 0..6, the baseline under row 6; row 7 takes the descenders of g j p q y and
the comma); columns 5..7 are blank, column 7 in every glyph, for spacing.  It is NOT OpenCV's FONT_HERSHEY_PLAIN, which the
reference's draw_caption uses: that is a stroke font; captions here have the same content and place, not the same pixels.
Digits, both letter cases, space and . : - _ % ( ) / + , # =; any other character draws as the hollow box BOX."""

CELL = 8      # a glyph's cell grid is CELL x CELL
ADVANCE = 6   # cells from one character's left edge to the next: 5 columns of ink and one of air
BASELINE = 7  # cell rows above the baseline (rows 0..6)

BOX = 0x001F11111111111F

GLYPHS = {
    ' ': 0x0000000000000000,
    '0': 0x000E11131519110E, '1': 0x000E040404040604, '2': 0x001F02040810110E, '3': 0x000E11100C10110E,
    '4': 0x0008081F090A0C08, '5': 0x000E1110100F011F, '6': 0x000E11110F01020C, '7': 0x000202020408101F,
    '8': 0x000E11110E11110E, '9': 0x000608101E11110E, 'A': 0x001111111F11110E, 'B': 0x000F11110F11110F,
    'C': 0x000E11010101110E, 'D': 0x0007091111110907, 'E': 0x001F01010F01011F, 'F': 0x000101010F01011F,
    'G': 0x001E11111D01110E, 'H': 0x001111111F111111, 'I': 0x000E04040404040E, 'J': 0x000609080808081C,
    'K': 0x0011090503050911, 'L': 0x001F010101010101, 'M': 0x0011111115151B11, 'N': 0x0011111119151311,
    'O': 0x000E11111111110E, 'P': 0x000101010F11110F, 'Q': 0x001609151111110E, 'R': 0x001109050F11110F,
    'S': 0x000F10100E01011E, 'T': 0x000404040404041F, 'U': 0x000E111111111111, 'V': 0x00040A1111111111,
    'W': 0x00111B1515111111, 'X': 0x0011110A040A1111, 'Y': 0x00040404040A1111, 'Z': 0x001F01020408101F,
    'a': 0x001E111E100E0000, 'b': 0x000F1111110F0101, 'c': 0x001E0101011E0000, 'd': 0x001E1111111E1010,
    'e': 0x000E011F110E0000, 'f': 0x000202020702120C, 'g': 0x0E101E11111E0000, 'h': 0x00111111110F0101,
    'i': 0x000E040404060004, 'j': 0x06090808080C0008, 'k': 0x0009050305090101, 'l': 0x000E040404040406,
    'm': 0x00151515150B0000, 'n': 0x00111111110F0000, 'o': 0x000E1111110E0000, 'p': 0x01010F11110F0000,
    'q': 0x10101E11111E0000, 'r': 0x00010101130D0000, 's': 0x000F100E011E0000, 't': 0x000C120202070202,
    'u': 0x001E111111110000, 'v': 0x00040A1111110000, 'w': 0x000A151511110000, 'x': 0x00110A040A110000,
    'y': 0x0E101E1111110000, 'z': 0x001F0204081F0000, '.': 0x0006060000000000, ':': 0x0000060600060600,
    '-': 0x000000001F000000, '_': 0x001F000000000000, '%': 0x00191A0204080B13, '(': 0x0008040202020408,
    ')': 0x0002040808080402, '/': 0x0001020204080810, '+': 0x000004041F040400, ',': 0x0204060600000000,
    '#': 0x000A0A1F0A1F0A0A, '=': 0x0000001F001F0000,
}

REQUIRED = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz .:-_%()/+,#="


def glyph(ch):
    """the 64-bit bitmap of one character (BOX for a character the font does not have)"""
    return GLYPHS.get(ch, BOX)


def glyph_words(ch):
    """(bits 0..31, bits 32..63) of glyph(ch) as two int32 values: fields a2, a3 of a GLYPH record"""
    v = glyph(ch)
    lo, hi = v & 0xFFFFFFFF, v >> 32
    return (lo - (1 << 32) if lo >= 1 << 31 else lo), (hi - (1 << 32) if hi >= 1 << 31 else hi)


def render(ch):
    """the glyph as eight strings of '#' and '.', to look at"""
    v = glyph(ch)
    return ["".join("#" if v >> (8 * r + c) & 1 else "." for c in range(CELL)) for r in range(CELL)]
