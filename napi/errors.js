'use strict';
// The C library's error codes as the addon throws them: an Error whose `code` is the decimal FSKHIP_E_* value and whose message is
// fskhip_last_error()'s (addon_util.h, throw_fsk).  The table is include/fskhip.h's enum and include/fskhip_next.h's defines, name
// by name -- one number space, every name a value of its own (tests/test_abi.py holds the headers, this table and the Python
// bindings together).  No addon is loaded here.
const ERRORS = Object.freeze({
  E_INVALID: -1, E_NOT_CONFIGURED: -2, E_UNSUPPORTED: -3, E_NO_DEVICE: -4, E_HIP: -5, E_NOMEM: -6, E_OVERFLOW: -7,
  E_BUSY: -8,      // 'Modulation already in progress' (fsk-processor.ts:90-92)
  E_HANDOFF: -9,   // a hand-off wait of a multi-wave kernel ran into its bound: the engine is to be destroyed
});
const codeOf = (e) => (e && typeof e.code === 'string' && /^-?\d+$/.test(e.code) ? Number(e.code) : null);

// What a call that can find a stream busy throws for the addon's error `e`: FSKHIP_E_BUSY, and no other code, becomes the
// reference's own Error with `text`; every other error -- FSKHIP_E_HANDOFF among them -- is handed on as it is.
function busyError(e, text) {
  return codeOf(e) === ERRORS.E_BUSY ? new Error(text) : e;
}

module.exports = { ERRORS, codeOf, busyError };
