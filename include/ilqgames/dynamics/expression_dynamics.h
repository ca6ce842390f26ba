// No counterpart in the reference (a user-defined model is a SinglePlayerDynamicalSystem subclass there): host::Expr and
// SinglePlayerExpressionSystem, the formula-defined model that runs on the device.  The mirrored declarations live in
// one header.
#include <ilqgames/host/api.hpp>
