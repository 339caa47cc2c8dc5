"""include/moviigen_hip.h read as ctypes: what every entry of wan.backend.lib's tables has to say.  A wrong entry there is silent memory
corruption, so the tables stay written out by hand and the tests compare them with this reading of the header."""
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'moviigen_hip.h')
SCALARS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float, 'double': ctypes.c_double}
RETURNS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'void': None, 'const char*': ctypes.c_char_p}


def header_declarations():
    """{name: (restype, [argtypes])} of every mg_* function the header declares (its MG_AB_BUILD section included), comments stripped:
    a pointer of any kind is c_void_p, int / int64_t / float / double are their ctypes, (void) is no argument."""
    hdr = re.sub(r'/\*.*?\*/', ' ', open(HEADER).read(), flags=re.S)
    hdr = re.sub(r'//[^\n]*', ' ', hdr)
    decl = {}
    for ret, name, args in re.findall(r'^(const\s+char\s*\*|int64_t|int|void)\s*(mg_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', hdr, re.M):
        assert name not in decl, f'{name} is declared twice'
        argtypes = []
        for arg in (' '.join(a.split()) for a in args.split(',')):
            if arg == 'void' and ',' not in args:
                continue
            if '*' in arg:
                argtypes.append(ctypes.c_void_p)
            else:
                ctype = arg.rsplit(' ', 1)[0].replace('const ', '')
                assert ctype in SCALARS, f'{name}: no ctypes mapping for the argument "{arg}"'
                argtypes.append(SCALARS[ctype])
        decl[name] = (RETURNS[re.sub(r'\s*\*', '*', ' '.join(ret.split()))], argtypes)
    return decl
